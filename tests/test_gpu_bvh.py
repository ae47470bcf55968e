"""GPU: BVH export - the kernels (csrc/k_bvh.hip through amuse_amd/bvh.py) against tests/bvh_ref.py (scipy's Rotation in float64, the unwrap rule in numpy,
Python's "%11.6f") on the seeded cases of tests/bvh_cases.py, their bitwise invariances, the file round trip and the paths built on them (amuse_amd.main --bvh,
python -m amuse_amd.bvh).

Bars.  Text: byte-exact.  Rotations: the geodesic angle between the rotation rebuilt from the EMITTED TEXT (scipy, the file's channel order) and
Rotation.from_rotvec of the fp32 input in float64, <= 1e-5 rad on every case, gimbal sets included - the project's usual parity bar, about 8 x what the fp32
restatement reaches (1.1e-6).  Channels, more than 1 degree from gimbal lock: within 4 x the fp32 restatement's own worst channel error on the same cases
(bvh_cases.euler_cases "margin": 2.3e-4 .. 6.7e-4 degrees depending on the order, plus the 0.5e-6 of the six-decimal rounding), modulo 360.  Unwrapped curves on
the crafted sequences: within 1e-3 degrees of the generating ones.  Measured on an MI355X: worst geodesic 8.3e-7 .. 1.17e-6 rad by order (gimbal sets 5.4e-7 ..
7.5e-7), channels away from lock 5.7e-5 .. 1.7e-4 degrees, unwrapped curves 2.8e-4 degrees, file round trip 1.3e-6 rad."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import body_cases as bc
import bvh_cases as cases
import bvh_ref as ref

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
DEV = "cuda:0"
BAR = 1e-5
DFS = ref.dfs(bc.make_model()["parents"])          # any column order serves the kernel tests: the synthetic model's tree


def _motion(poses, frames, order="ZYX", trans=None, root_rest=None, scale=100.0, unwrap=False, euler=True, text=True):
    from amuse_amd import bvh
    S = len(frames)
    rr = np.zeros((S, 3), np.float32) if root_rest is None else root_rest
    e, t, st = bvh.motion_channels(torch.tensor(poses, device=DEV), None if trans is None else torch.tensor(trans, device=DEV), torch.tensor(rr), frames, DFS,
                                   order, scale, unwrap, euler=euler, text=text)
    torch.cuda.synchronize()
    return (None if e is None else e.cpu().numpy()), (None if t is None else t.cpu().numpy().tobytes()), st.cpu().numpy()


def _joint_channels(block):
    """text block -> (rows, 55, 3) degrees in SMPL-X joint order"""
    v = ref.parse(block)[:, 3:].reshape(-1, 55, 3)
    out = np.empty_like(v)
    out[:, DFS] = v
    return out


# ------------------------------------------------------------------ the formatter
@pytest.mark.parametrize("n", [1, 167, 169, 4096])
def test_formatter_is_printf(n):
    from amuse_amd import bvh
    v = cases.format_values()[4096 - n:]                      # (the tail holds the edge values: every n sees some)
    text, status = bvh.format_values(torch.tensor(v, device=DEV), 168)
    torch.cuda.synchronize()
    got, want = text.cpu().numpy().tobytes(), ref.fmt(v, 168)
    assert len(got) == 12 * n and int(status.item()) == 0
    if got != want:
        bad = [i for i in range(n) if got[12 * i:12 * i + 12] != want[12 * i:12 * i + 12]]
        raise AssertionError(f"{len(bad)} fields differ; first: value {v[bad[0]]!r} got {got[12 * bad[0]:12 * bad[0] + 12]!r} want {want[12 * bad[0]:12 * bad[0] + 12]!r}")


def test_formatter_out_of_range_and_canary():
    from amuse_amd import _lib
    import ctypes as C
    v = cases.format_values()[:200].copy()
    bad = {5: 1000.0, 17: float("nan"), 40: float("inf"), 41: -float("inf"), 167: -1000.0}
    for i, x in bad.items():
        v[i] = x
    n = v.size
    buf = torch.full((12 * n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    vals = torch.tensor(v, device=DEV)
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert _lib.load().amuse_bvh_format(vp(vals), n, 168, vp(buf), vp(status), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy().tobytes()
    assert got[12 * n:] == b"\xa5" * 64                                             # the canary behind the buffer
    assert status.cpu().tolist() == [1, 0]
    for i in range(n):
        field, sep = got[12 * i:12 * i + 11], got[12 * i + 11:12 * i + 12]
        assert sep == (b"\n" if i % 168 == 167 else b" ")
        if i in bad:
            assert field == b"#" * 11, (i, field)
        else:
            assert field == b"%11.6f" % float(v[i]), (i, field)                      # the neighbours are exact
    # all in range: the status stays clear
    status.zero_()
    vals = torch.tensor(cases.format_values()[:200], device=DEV)
    assert _lib.load().amuse_bvh_format(vp(vals), n, 168, vp(buf), vp(status), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0]


# ------------------------------------------------------------------ Euler channels, principal values
@pytest.mark.parametrize("order", ref.ORDERS)
def test_principal_channels_against_scipy(order):
    c = cases.euler_cases(order)
    poses = c["aa"].reshape(40, 55, 3)
    euler, text, status = _motion(poses, cases.FRAMES3, order)
    assert not status.any() and len(text) == 40 * 2016
    deg = _joint_channels(text).reshape(-1, 3)
    assert np.array_equal(ref.parse(text), np.array([float("%.6f" % x) for x in euler.reshape(-1)]).reshape(40, 168))      # the tap is what the text states
    g = ref.geodesic(c["aa"], deg, order)
    for name, sl in c["cls"].items():
        print(f"{order} {name}: geodesic max {g[sl].max():.3e} rad")
    print(f"{order}: geodesic max {g.max():.3e} rad (fp32 restatement {c['f32_geo']:.3e}, bar {BAR:.0e})")
    assert g.max() <= BAR, {n: float(g[s].max()) for n, s in c["cls"].items()}
    assert np.abs(deg[:, 1]).max() <= 90.0 and np.abs(deg[:, [0, 2]]).max() <= 180.0
    err = np.abs(ref.mod360(deg - c["ref"]))[c["away"]]
    print(f"{order}: channels away from lock, worst {err.max():.3e} deg (margin {c['margin']:.3e})")
    assert err.max() <= c["margin"] + 0.5e-6, (float(err.max()), c["margin"])
    assert np.abs(ref.parse(text)[:, :3]).max() == 0.0                              # root_rest 0, no trans


def test_clip_of_300_frames_with_translation():
    c = cases.clip300()
    rr = np.array([[0.0123, -0.345, 0.0271]], np.float32)
    euler, text, status = _motion(c["poses"], [300], "ZYX", trans=c["trans"], root_rest=rr)
    assert not status.any() and text == ref.fmt(euler, 168)
    g = ref.geodesic(c["poses"], _joint_channels(text).reshape(-1, 3), "ZYX")
    print(f"clip300: geodesic max {g.max():.3e} rad")
    assert g.max() <= BAR
    want = ((rr.astype(np.float32) + c["trans"]) * np.float32(100.0)).astype(np.float32)
    assert np.array_equal(euler[:, :3], want)
    # text alone, the tap alone: the same values
    assert _motion(c["poses"], [300], "ZYX", trans=c["trans"], root_rest=rr, euler=False)[1] == text
    assert np.array_equal(_motion(c["poses"], [300], "ZYX", trans=c["trans"], root_rest=rr, text=False)[0].view(np.uint32), euler.view(np.uint32))


# ------------------------------------------------------------------ unwrap
@pytest.mark.parametrize("order", ref.ORDERS)
def test_unwrap_returns_the_generating_curves(order):
    for case, jump in ((cases.spin(order), 340.0), (cases.fold(order), 180.0)):
        F = case["poses"].shape[0]
        _, plain, st0 = _motion(case["poses"], [F], order)
        _, text, st1 = _motion(case["poses"], [F], order, unwrap=True)
        assert not st0.any() and not st1.any()
        p, u = _joint_channels(plain), _joint_channels(text)
        assert np.abs(np.diff(p, axis=0)).max() > jump - 1.0                       # unwrap off: the jumps are there, the case discriminates
        assert np.abs(np.diff(u, axis=0)).max() <= 180.0
        d = np.abs(u - case["curves"]).max()
        print(f"{order}: unwrapped curves within {d:.3e} deg of the generating ones")
        assert d <= 1e-3
        assert ref.geodesic(case["poses"], u.reshape(-1, 3), order).max() <= BAR   # the same rotations
        assert np.abs(u - ref.unwrap(p)).max() <= 1e-3                            # and the float64 rule on the kernel's own principal values


def test_unwrap_on_mixed_rotations_and_text_only_staging():
    """40 frames of UNRELATED rotations: the walk still emits the same rotations with steps <= 180 degrees; a column that winds past 1000 degrees on the way is
    '#' in the text and sets its sequence's status - the tap keeps the value"""
    c = cases.euler_cases("ZYX")
    poses = c["aa"].reshape(40, 55, 3)
    euler, text, status = _motion(poses, cases.FRAMES3, "ZYX", unwrap=True)
    assert text == ref.fmt(euler, 168)
    u = np.empty((40, 55, 3))
    u[:, DFS] = euler[:, 3:].reshape(40, 55, 3)
    # rebuilt from what the text states: the joints all three of whose channels fit the field (a wound value of thousands of degrees has an fp32 spacing of
    # 2.4e-4 degrees and more; it is '#' in the file)
    fits = (np.abs(u) < 999.9999995).all(-1)
    g = ref.geodesic(c["aa"].reshape(40, 55, 3)[fits], np.round(u[fits], 6), "ZYX")
    print(f"unwrap, mixed: {fits.sum()} of {fits.size} joints fit the field; geodesic max {g.max():.3e} rad; largest channel {np.abs(u).max():.1f} deg")
    assert fits.mean() > 0.5 and g.max() <= BAR
    o = 0
    for s, F in enumerate(cases.FRAMES3):
        if F > 1:
            step = np.abs(np.diff(u[o:o + F], axis=0)).max()
            print(f"unwrap, mixed: sequence {s} largest step {step:.6f} deg")
            assert step <= 180.0 + 2.0 ** -11                   # (the fp32 spacing of the wound values: 2^-12 below 4096 degrees, on either end of a step)
        assert bool(status[s]) == (b"#" in text[o * 2016:(o + F) * 2016])
        o += F
    # without the tap the principal values wait in the text buffer itself: the same bytes
    assert _motion(poses, cases.FRAMES3, "ZYX", unwrap=True, euler=False)[1] == text
    # 300 frames of a periodic motion with the tap and without it; a joint that circles a gimbal pole once per period winds by 360 degrees each time, so the
    # status may be set here too - the bytes and the rotations that the text states are held either way
    c3 = cases.clip300()
    e3, t3, s3 = _motion(c3["poses"], [300], "ZYX", trans=c3["trans"], unwrap=True)
    assert t3 == ref.fmt(e3, 168) and _motion(c3["poses"], [300], "ZYX", trans=c3["trans"], unwrap=True, euler=False)[1] == t3 and bool(s3[0]) == (b"#" in t3)
    u3 = np.empty((300, 55, 3))
    u3[:, DFS] = e3[:, 3:].reshape(300, 55, 3)
    fits = (np.abs(u3) < 999.9999995).all(-1)
    g = ref.geodesic(c3["poses"][fits], np.round(u3[fits], 6), "ZYX")
    print(f"unwrap, clip300: {fits.sum()} of {fits.size} joints fit the field; geodesic max {g.max():.3e} rad; largest channel {np.abs(u3).max():.1f} deg")
    assert fits.mean() > 0.9 and g.max() <= BAR and np.abs(np.diff(u3, axis=0)).max() <= 180.0 + 2.0 ** -11


def test_winding_past_1000_degrees_sets_its_own_status_only():
    w, c = cases.wind("ZYX")["poses"], cases.euler_cases("ZYX")["aa"].reshape(40, 55, 3)
    a, b = c[:2], c[2:3]
    _, text, status = _motion(np.concatenate([a, w, b]), [2, 37, 1], "ZYX", unwrap=True)
    assert status.tolist() == [0, 1, 0]
    _, alone, st = _motion(np.concatenate([a, b]), [2, 1], "ZYX", unwrap=True)
    assert not st.any() and text[:2 * 2016] == alone[:2 * 2016] and text[39 * 2016:] == alone[2 * 2016:]
    mid = text[2 * 2016:39 * 2016]
    assert b"#" * 11 in mid and b"#" not in alone and b"#" not in mid[:6 * 2016]                # the first six frames stay below 1000
    _, plain, st = _motion(np.concatenate([a, w, b]), [2, 37, 1], "ZYX")
    assert not st.any() and b"#" not in plain                                                    # the remedy: without unwrap it fits
    # the position channels: a scale that does not fit
    _, t2, st = _motion(np.concatenate([a, b]), [2, 1], "ZYX", trans=np.float32([[0, 0, 0], [0, 11.0, 0], [0, 0, 0]]))
    assert st.tolist() == [1, 0] and t2[2016 + 12:2016 + 23] == b"#" * 11 and t2[2 * 2016:] == alone[2 * 2016:]


# ------------------------------------------------------------------ invariance
def test_batch_position_and_graph_replay():
    from amuse_amd import bvh
    c = cases.euler_cases("YZX")
    poses = c["aa"].reshape(40, 55, 3)
    g = np.random.default_rng(5)
    trans, rr = g.standard_normal((40, 3)).astype(np.float32), g.standard_normal((3, 3)).astype(np.float32) * 0.3
    for unwrap in (False, True):
        euler, text, st = _motion(poses, cases.FRAMES3, "YZX", trans=trans, root_rest=rr, unwrap=unwrap)
        assert bool(st.any()) == (b"#" in text) and not (st.any() and not unwrap)
        e2, t2, _ = _motion(poses[3:], [37], "YZX", trans=trans[3:], root_rest=rr[2:], unwrap=unwrap)                  # third in the batch == alone
        assert t2 == text[3 * 2016:] and np.array_equal(e2.view(np.uint32), euler[3:].view(np.uint32))
        # 33 sequences: the last one sits in a second launch
        many_p, many_t = np.concatenate([poses[:1]] * 32 + [poses[3:]]), np.concatenate([trans[:1]] * 32 + [trans[3:]])
        _, t33, _ = _motion(many_p, [1] * 32 + [37], "YZX", trans=many_t, root_rest=np.concatenate([rr[:1]] * 32 + [rr[2:]]), unwrap=unwrap)
        assert t33[32 * 2016:] == t2 and t33[:2016] == text[:2016]
        # the tap formatted by the formatter on its own == the text
        ft, fs = bvh.format_values(torch.tensor(euler, device=DEV), 168)
        assert ft.cpu().numpy().tobytes() == text and bool(fs.item()) == bool(st.any())
        # a captured call replayed on overwritten inputs == eager
        p, t, r = torch.tensor(poses, device=DEV), torch.tensor(trans, device=DEV), torch.tensor(rr, device=DEV)
        call = lambda: bvh.motion_channels(p, t, r, cases.FRAMES3, DFS, "YZX", 100.0, unwrap, euler=True, text=True)
        call()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            ge, gt, gs = call()
        gr.replay()
        torch.cuda.synchronize()
        assert gt.cpu().numpy().tobytes() == text
        p.copy_(p.flip(0) * 0.9)
        gr.replay()
        torch.cuda.synchronize()
        ee, et, _ = call()
        torch.cuda.synchronize()
        assert torch.equal(gt, et) and torch.equal(ge, ee) and gt.cpu().numpy().tobytes() != text


# ------------------------------------------------------------------ the file round trip
@pytest.mark.parametrize("order,scale", [("ZYX", 100.0), ("XZY", 1.0)])
def test_file_round_trip(tmp_path, order, scale):
    """write_bvh -> read_bvh -> amuse_bvh_decode.  The translation bound: the position p = (rest + trans) x scale is printed at six decimals (<= 0.5e-6 in file
    units, 0.5e-6 / scale in metres) and passes through fp32 five times (the sum, the product, the reader's cast, the quotient, the difference), each within
    2^-24 of max(|rest| + |trans|): |error| <= 0.5e-6 / scale + 5 x 2^-24 x (|rest| + |trans|)_max."""
    from amuse_amd import bvh
    from amuse_amd.body import BodyModel
    m = BodyModel.from_dict(bc.make_model())
    betas = bc.make_betas(1)[0]
    J = bvh.rest_joints(m, betas)
    dfs = bvh.layout(m.parents)
    assert list(dfs) == DFS
    c = cases.clip300()
    poses, trans = c["poses"][:37], c["trans"][:37]
    rr = J[:1].astype(np.float32)
    _, text, status = bvh.motion_channels(torch.tensor(poses, device=DEV), torch.tensor(trans, device=DEV), torch.tensor(rr), [37], dfs, order, scale)
    assert not status.cpu().numpy().any()
    p = bvh.write_bvh(tmp_path / "a_motion.bvh", bvh.header_text(m.parents, J, 37, 30.0, order, scale), text.cpu().numpy().tobytes())
    b = bvh.read_bvh(p)
    assert b["frames"] == 37 and b["order"] == order and list(b["dfs"]) == DFS and b["meta"] is None          # the column order is the depth-first order
    want = np.zeros((55, 3))
    want[1:] = (J[1:] - J[m.parents[1:]]) * scale
    assert np.array_equal(b["offsets"], np.array([[float("%.6f" % x) for x in row] for row in want]))         # the rest-joint differences x scale at six decimals
    po, to = bvh.decode(torch.tensor(b["channels"].astype(np.float32), device=DEV), [37], b["dfs"], b["order"], scale, rr)
    torch.cuda.synchronize()
    po, to = po.cpu().numpy(), to.cpu().numpy()
    g = ref.geodesic_aa(poses, po)
    tb = 0.5e-6 / scale + 5 * 2.0 ** -24 * float(np.abs(rr).max() + np.abs(trans).max())
    terr = np.abs(to.astype(np.float64) - trans)
    print(f"{order} scale {scale}: round trip geodesic max {g.max():.3e} rad; trans error {terr.max():.3e} (bound {tb:.3e})")
    assert g.max() <= BAR and np.linalg.norm(po, axis=-1).max() <= np.pi + 1e-6
    assert terr.max() <= tb
    # the decoder on the hard cases: every class, gimbal sets included
    e = cases.euler_cases(order)
    euler, _, _ = bvh.motion_channels(torch.tensor(e["aa"].reshape(40, 55, 3), device=DEV), None, torch.zeros(3, 3), cases.FRAMES3, dfs, order, scale, text=False, euler=True)
    po, to = bvh.decode(euler, cases.FRAMES3, dfs, order, scale, torch.zeros(3, 3))
    g = ref.geodesic_aa(e["aa"], po.cpu().numpy())
    print(f"{order}: decode of the case set, geodesic max {g.max():.3e} rad")
    assert g.max() <= BAR and not to.cpu().numpy().any() and np.linalg.norm(po.cpu().numpy(), axis=-1).max() <= np.pi + 1e-6


# ------------------------------------------------------------------ the product
def _models(path):
    from amuse_amd.body import BodyModel
    path.mkdir(parents=True, exist_ok=True)
    for i, name in enumerate(("SMPLX_MALE.npz", "SMPLX_FEMALE.npz", "SMPLX_NEUTRAL.npz")):
        BodyModel.from_dict(bc.make_model(V=203, seed=i)).to_npz(path / name)
    return path


def _run(args, **kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "AMUSE_RUN_STAMP")}
    env.update(AMUSE_RUN_STAMP="20260101-000000")
    return subprocess.run([sys.executable, "-m", *args], cwd=REPO, env=env, capture_output=True, text=True, timeout=900, **kw)


def test_cli_bvh(tmp_path):
    from conftest import make_reference_tree
    from amuse_amd import body, bvh
    from amuse_amd.npz_writer import LOWER_BODY_JOINTS
    models = _models(tmp_path / "models")
    base = lambda root: ["amuse_amd.main", "--fn", "infer_gesture", "--root", str(root), "--random-init"]
    files = lambda root: sorted(p for p in root.rglob("*") if p.is_file() and p.suffix in (".npz", ".bvh", ".json") and "viz_dump" in p.parts)
    ra, rb = make_reference_tree(tmp_path / "a", n_infer_wavs=2), make_reference_tree(tmp_path / "b", n_infer_wavs=2)
    r = _run(base(ra))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    r = _run(base(rb) + ["--bvh", "--smplx-models", str(models), "--bvh-order", "YXZ"])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    a, b = files(ra), files(rb)
    npz = [p for p in b if p.suffix == ".npz"]
    bvhs = [p for p in b if p.suffix == ".bvh"]
    assert not [p for p in a if p.suffix != ".npz"] and len(a) == len(npz) == len(bvhs) == 2                 # off by default; one .bvh per NPZ
    assert [p.relative_to(ra) for p in a] == [p.relative_to(rb) for p in npz]
    assert all(p.read_bytes() == q.read_bytes() for p, q in zip(a, npz))                                     # the NPZ files keep their bytes
    loaded = body.load_models(models)
    for n, f in zip(npz, bvhs):
        assert f.name == n.name.replace("_motion_smplx.npz", "_motion.bvh")
        d = bvh.read_bvh(f)
        with np.load(n) as z:
            poses, gender, betas = z["poses"], str(z["gender"]), z["betas"]
        assert d["frames"] == 300 and d["order"] == "YXZ" and d["meta"]["gender"] == gender and np.array_equal(d["meta"]["betas"], betas)
        J = bvh.rest_joints(loaded[gender], betas)
        assert np.allclose(d["meta"]["root_rest"], J[0], atol=0, rtol=0)
        po, to = bvh.decode(torch.tensor(d["channels"].astype(np.float32), device=DEV), [300], d["dfs"], "YXZ", 100.0, J[:1].astype(np.float32))
        po = po.cpu().numpy()
        assert ref.geodesic_aa(poses, po).max() <= BAR                                                       # the BVH holds what the NPZ holds ...
        assert ref.geodesic_aa(po[:, LOWER_BODY_JOINTS], np.broadcast_to(po[:1, LOWER_BODY_JOINTS], (300, 8, 3))).max() <= 1e-7       # ... the lower-body freeze included
        assert np.abs(to.cpu().numpy()).max() <= 0.5e-8 + 5 * 2.0 ** -24 * float(np.abs(J[0]).max())
    # the tool on those NPZ files: the same bytes; and back
    r = _run(["amuse_amd.bvh", *map(str, npz), "--smplx-models", str(models), "-o", str(tmp_path / "out"), "--order", "YXZ"])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    for f in bvhs:
        assert (tmp_path / "out" / f.name).read_bytes() == f.read_bytes() and (tmp_path / "out" / (f.name + ".json")).read_bytes() == (f.parent / (f.name + ".json")).read_bytes()
    r = _run(["amuse_amd.bvh", "--to-npz", *(str(tmp_path / "out" / f.name) for f in bvhs), "-o", str(tmp_path / "back")])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    for n in npz:
        with np.load(tmp_path / "back" / n.name.replace("_motion_smplx.npz", "_from_bvh_motion_smplx.npz")) as zb, np.load(n) as z:
            assert zb["poses"].shape == (300, 55, 3) and ref.geodesic_aa(zb["poses"], z["poses"]).max() <= BAR and np.abs(zb["trans"]).max() <= 1e-6
            assert str(zb["gender"]) == str(z["gender"]) and np.array_equal(zb["betas"], z["betas"]) and float(zb["mocap_frame_rate"]) == float(z["mocap_frame_rate"])
    r = _run(base(rb) + ["--bvh-order", "XYZ"])
    assert r.returncode != 0 and "belong to --bvh" in r.stderr
