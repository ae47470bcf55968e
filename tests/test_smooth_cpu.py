"""CPU: motion smoothing without a GPU - the bank the library computes (amuse_smooth_banks, host only) against tests/smooth_ref.py's float64 restatement and
against scipy.signal, the restatement's own properties (what the header claims of the method), the seeded cases' branch coverage, the ABI and the argument
parsing.  The filter itself is a HIP kernel: tests/test_gpu_smooth.py.

Bars.  Bank: <= 1 ulp of fp32 against the restatement rounded to fp32 (two double computations of the same matrix, by Gram-Schmidt and by QR, agree to 1e-15;
only a value that sits on a rounding boundary can land on the neighbouring float; values below 2^-20 - the 1e-17 leftovers of the H = I cases - are measured
in ulps of 2^-20).  scipy: savgol_coeffs solves the same least-squares problem in double on
the UNSCALED abscissae -m .. m (a Vandermonde matrix of condition number up to 5e5 at m = 15, order 5) and is the less accurate side (it sits 1.4e-9 from the
QR form at m = 13, order 5, 1e-12 and less at order <= 3); the bar is 1e-8 absolute, a sixth of the 2^-24 the bank is then rounded to.  Translation against savgol_filter(mode="interp"): 1e-6 on |x| ~ 1,
the fp32 rounding of the bank (2^-24 per coefficient, up to 31 of them) - the restatement uses the bank the kernel uses."""
import re
from pathlib import Path

import numpy as np
import pytest

import smooth_cases as cases
import smooth_ref as ref

REPO = Path(__file__).resolve().parents[1]


def _banks(order):
    from amuse_amd import smooth
    return smooth.banks(order)


@pytest.mark.parametrize("order", range(6))
def test_bank_against_restatement_and_scipy(order):
    from scipy.signal import savgol_coeffs
    bk = _banks(order)
    assert bk.shape == (ref.BANK_FLOATS,) and bk.dtype == np.float32
    want = ref.banks(order)
    ulp = np.abs(bk.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.float32(2.0 ** -20)))
    print(f"order {order}: bank worst {ulp.max():.2f} ulp of fp32 against the restatement (values differing: {int((bk != want).sum())} of {bk.size})")
    assert ulp.max() <= 1.0
    worst = 0.0
    for m in range(1, ref.MAX_HALF + 1):
        H, n, pm = ref.bank_of(bk, m), 2 * m + 1, min(order, 2 * m)
        assert np.abs(H.sum(1, dtype=np.float64) - 1.0).max() <= 1e-6, m                      # rows sum to 1: a constant is reproduced
        H64 = ref.hat(m, order)
        bar = 1e-8
        if pm < 2 * m:      # the header's formula, taken literally
            assert np.abs(H64 - ref.hat_normal_equations(m, order)).max() <= bar, m
        for r in range(n):
            c = savgol_coeffs(n, pm, pos=r, use="dot")
            worst = max(worst, float(np.abs(H64[r] - c).max()))
            assert np.abs(H64[r] - c).max() <= bar and np.abs(H[r].astype(np.float64) - c).max() <= 2.0 ** -23, (m, r)
    print(f"order {order}: restatement against scipy.signal.savgol_coeffs, every row of every m: {worst:.2e}")


def test_bank_refuses_bad_arguments_and_is_declared():
    from amuse_amd import _lib, smooth
    lib = _lib.load()
    hdr = (REPO / "include" / "amuse_hip.h").read_text()
    for name in ("amuse_smooth_banks", "amuse_smooth_motion"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.EXPORTS and hasattr(lib, name)
    for order in (-1, 6):
        with pytest.raises(_lib.AmuseHipError):
            smooth.banks(order)
    assert lib.amuse_smooth_banks(3, None) != 0
    assert [smooth.bank_offset(m) for m in (1, 2, 3, 16)] == [0, 9, 34, ref.BANK_FLOATS] == [ref.bank_offset(m) for m in (1, 2, 3, 16)]
    H4 = ref.bank_of(smooth.banks(3), 4)
    # the classic central kernel of window 9, order 3: (-21, 14, 39, 54, 59, 54, 39, 14, -21) / 231
    assert H4.shape == (9, 9) and np.abs(H4[4] * 231 - np.array([-21, 14, 39, 54, 59, 54, 39, 14, -21])).max() < 1e-4


@pytest.mark.parametrize("m,p", [(1, 1), (4, 3), (15, 5), (7, 2), (2, 5)])
def test_translation_restatement_is_savgol_interp(m, p):
    from scipy.signal import savgol_filter
    rng = np.random.default_rng(m * 10 + p)
    for L in (2 * m + 1, 2 * m + 2, 97):
        x = rng.standard_normal((L, 3)).astype(np.float32)
        want = savgol_filter(x.astype(np.float64), 2 * m + 1, min(p, 2 * m), axis=0, mode="interp")
        exact = ref.filter_vectors(x, ref.hat(m, p))            # (the float64 matrix, rounded to fp32 inside: the bank's own rounding is the difference)
        got = ref.filter_vectors(x, ref.bank_of(ref.banks(p), m))
        assert np.array_equal(exact, got)
        err = float(np.abs(got - want).max())
        print(f"m {m} p {p} L {L}: restatement (fp32 bank) against scipy.signal.savgol_filter(mode='interp'): {err:.2e}")
        assert err <= 1e-6
    # with the bank left in double the two agree to double rounding
    H = ref.hat(m, p)
    s, r = ref.window_of(97, m)
    x = rng.standard_normal((97, 3))
    mine = sum(H[r, k][:, None] * x[s + k] for k in range(2 * m + 1))
    err = float(np.abs(mine - savgol_filter(x, 2 * m + 1, min(p, 2 * m), axis=0, mode="interp")).max())
    print(f"m {m} p {p}: float64 bank against scipy.signal.savgol_filter(mode='interp'): {err:.2e}")
    assert err <= 1e-8 * (2 * m + 1) * np.abs(x).max()          # the coefficient bar of the bank test, over a window


def test_cases_reach_every_branch():
    c = cases.mixed()
    assert c["poses"].shape == (sum(cases.MIXED_FRAMES), 55, 3) and c["f32_dist"] < 2e-6 and c["bar"] < 1e-5
    print(f"mixed: {len(c['frames'])} sequences, {c['poses'].shape[0]} frames, float32 restatement {c['f32_dist']:.2e} rad, translation {c['t32_dist']:.2e}")
    # not filtered: the input's values
    keep = ~c["mask"][:, :55]
    assert np.array_equal(c["p64"][keep], c["poses"][keep].astype(np.float64)) and np.array_equal(c["t64"][~c["mask"][:, 55]], c["trans"][~c["mask"][:, 55]])
    assert np.linalg.norm(c["p64"][c["mask"][:, :55]], axis=-1).max() <= np.pi + 1e-12       # smoothed rows carry the short representation
    assert np.linalg.norm(c["p64"][keep], axis=-1).max() > np.pi                              # copied rows stay as they are


def test_restatement_reproduces_a_constant_and_folds_beyond_pi():
    rng = np.random.default_rng(3)
    one = rng.standard_normal((1, 55, 3))
    one *= rng.uniform(0.1, 3.0, (1, 55, 1)) / np.linalg.norm(one, axis=-1, keepdims=True)
    one[0, 0] = np.array([0.0, 3.5, 0.0])
    poses = np.repeat(one, 61, 0).astype(np.float32)
    out, _, _ = ref.smooth(poses, None, (61,), (4,) * 56, ref.banks(3))
    g = ref.geodesic(out, poses.astype(np.float64))
    print(f"constant: geodesic {g.max():.2e} rad")
    assert g.max() <= 1e-14
    assert np.abs(out[:, 0] - np.array([0.0, -(2 * np.pi - np.float64(np.float32(3.5))), 0.0])).max() <= 1e-12      # 3.5 rad comes out as 2 pi - 3.5 the other way


def test_restatement_reproduces_a_cubic_angle():
    """an order-3 fit reproduces a cubic: with exact inputs only the bank's rounding to fp32 is left - at most sum_k |H[r][k]| 2^-25 x the angle span of a
    window (below 2 rad) - and with fp32 inputs their own rounding, 2^-24 x 3.95 rad per component, filtered"""
    c = cases.cubic()
    H = ref.bank_of(c["bank"], 4)
    gain = float(np.abs(H.astype(np.float64)).sum(1).max())
    g_exact = ref.geodesic(ref.filter_rotations(c["exact"], H), c["exact"])
    g = ref.geodesic(c["p64"], c["exact"])
    print(f"cubic: exact inputs {g_exact.max():.2e} rad (bar {gain * 2.0 ** -25 * 2.0:.2e}); fp32 inputs {g.max():.2e}; float32 restatement "
          f"{c['f32_dist_exact']:.2e} from the analytic rotations")
    assert g_exact.max() <= gain * 2.0 ** -25 * 2.0 + 1e-12
    assert g.max() <= gain * 2.0 ** -25 * 2.0 + (1.0 + gain) * np.sqrt(3.0) * 2.0 ** -24 * 3.95 + 1e-12
    assert np.linalg.norm(c["exact"], axis=-1).max() > 3.9 and np.linalg.norm(c["p64"], axis=-1).max() <= np.pi + 1e-12


def test_restatement_is_left_equivariant():
    c = cases.noisy()
    g = ref.aa_to_quat(np.array([0.3, -1.1, 0.8]))
    left = lambda aa: ref.quat_to_aa(ref.qmul(np.broadcast_to(g, aa.shape[:-1] + (4,)), ref.aa_to_quat(aa)))
    H = ref.bank_of(c["bank"], 4)
    poses = c["poses"].astype(np.float64)
    a, b = ref.filter_rotations(poses, H), ref.filter_rotations(left(poses), H)
    err = ref.geodesic(left(a), b)
    print(f"left-multiplying every frame by one rotation left-multiplies the output: {err.max():.2e} rad")
    assert err.max() <= 1e-13 and ref.geodesic(a, poses).max() > 1e-3
    assert np.array_equal(a, c["p64"])


def test_restatement_smooths_a_noisy_motion():
    c = cases.noisy()
    (j_in, j_out), (d_in, d_out) = cases.noisy_inequalities(c, c["p64"])
    j_clean = cases.second_difference(c["clean"][:, c["score"]])
    print(f"noisy: mean geodesic second difference {j_in:.4f} -> {j_out:.4f} (clean {j_clean:.4f}); distance from the clean motion {d_in:.4f} -> {d_out:.4f}")
    assert j_out < j_in and d_out < d_in


def test_half_windows_and_argument_parsing():
    from amuse_amd import smooth
    assert smooth.half_windows() == [4] * 56
    hw = smooth.half_windows(9, 5)
    assert len(hw) == 56 and hw[:25] == [4] * 25 and hw[25:55] == [2] * 30 and hw[55] == 4
    assert smooth.half_windows(31)[0] == 15 and smooth.half_windows(3, 31)[30] == 15
    for bad in (1, 2, 8, 33, -9, 0):
        with pytest.raises(ValueError):
            smooth.half_windows(bad)
        with pytest.raises(ValueError):
            smooth.half_windows(9, bad)
    assert smooth.options() == {"window": 9, "order": 3} and smooth.options(5, 0, 7) == {"window": 5, "order": 0, "hands_window": 7}
    for bad in (-1, 6):
        with pytest.raises(ValueError):
            smooth.options(9, bad)
    a = smooth.parse_args(["a_motion_smplx.npz", "b.npz", "-o", "out", "--window", "11", "--order", "2", "--hands-window", "5"])
    assert a.files == ["a_motion_smplx.npz", "b.npz"] and (a.out_dir, a.window, a.order, a.hands_window) == ("out", 11, 2, 5)
    a = smooth.parse_args(["x.npz"])
    assert (a.window, a.order, a.hands_window, a.out_dir) == (9, 3, None, None)
    for bad in (["x.npz", "--window", "1"], ["x.npz", "--window", "10"], ["x.npz", "--order", "6"], ["x.npz", "--hands-window", "33"], []):
        with pytest.raises(SystemExit):
            smooth.parse_args(bad)
    assert smooth.output_path(Path("d/scott_seq_0_AbCdEf_motion_smplx.npz")).name == "scott_seq_0_AbCdEf_smoothed_motion_smplx.npz"
    assert smooth.output_path(Path("d/other.npz"), Path("o")) == Path("o/other_smoothed_motion_smplx.npz")
    import torch
    from amuse_amd import _lib
    with pytest.raises(_lib.AmuseHipError, match="no CPU fallback"):
        smooth.smooth(torch.zeros(9, 55, 3), None, [9])


@pytest.mark.parametrize("argv,msg", [
    (["--smooth", "--smooth-window", "1"], "--smooth"), (["--smooth", "--smooth-window", "10"], "--smooth"), (["--smooth", "--smooth-window", "33"], "--smooth"),
    (["--smooth", "--smooth-order", "6"], "--smooth"), (["--smooth", "--smooth-hands-window", "2"], "--smooth"), (["--smooth-window", "9"], "belong to --smooth")])
def test_main_rejects_bad_smoothing_switches(argv, msg):
    from amuse_amd import main as cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--fn", "infer_gesture", "--root", "/nonexistent"] + argv)
    assert msg in str(e.value)
