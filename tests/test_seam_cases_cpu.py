"""CPU: the seam-cost restatement's own properties (tests/seam_ref.py on tests/seam_cases.py) - the numbers the GPU tests are held to must be right before
anything is compared with them - and the dynamic programme against brute force over all K^W paths."""
import itertools

import numpy as np

import seam_cases as sc
import seam_ref as ref


def _two_windows(K=3, seed=0):
    F, hop = 12, 9
    poses, trans = sc.make(F, hop, (2,), (21,), K, seed)
    u, w, tw = sc.weights(F, hop)
    return F, hop, poses, trans, u, w, tw


def test_cases_are_what_the_docstring_says():
    c = sc.case("cut_short")
    F, hop, K = c["F"], c["hop"], c["K"]
    assert [Ok for _, Ok in ref.seams_of(c["windows"], c["frames"], F, hop)] == [3, 3, 1, 3, 3, 1]
    assert len(sc.CASES["capacity_plus_one"][2]) == sc.CAP + 1 and 1 in sc.CASES["capacity_plus_one"][2]
    assert (c["joint_weight"] == 0).sum() == 6 and len(set(c["row_weight"].tolist())) > 1
    cls = np.arange(55) % sc.N_CLASSES
    th = c["th64"][0]                                      # (K, K, 3, 55)
    assert th[..., cls == 0].max() > 3.0                   # beyond-pi inputs: angles near pi occur (theta itself is <= pi)
    assert (np.linalg.norm(c["poses"], axis=-1) > np.pi).any()
    assert th[..., cls == 1].max() < 1e-15                 # (w y + x z) - y w leaves a rounding of x z: amuse_rot.hpp's association, kept
    assert 1e-5 < th[..., cls == 2].max() < 1e-3 and 1e-3 < th[..., cls == 3].max() < 1e-1
    assert th[..., cls == 4].max() < 2e-6                  # the alias: the same rotation up to the fp32 rounding of the inputs
    assert th[..., cls == 5].max() < 2e-6 and th[..., cls == 5].max() > 0
    a, b = c["poses"][0:K, hop:hop + 3][:, :, cls == 6], c["poses"][K:2 * K, :3][:, :, cls == 6]
    assert not a[0].any() and a[1].any() and not b[0].any() and b[1].any()      # exact zeros: both sides at (0, 0), one side elsewhere
    for name in sc.CASES:
        k = sc.case(name)
        print(f"{name}: float32 restatement's largest |theta - theta64| {k['f32_dist']:.3e} rad, delta {k['delta']:.3e}")
        assert 0 < k["f32_dist"] < 1e-6 and k["cost64"].shape == (sum(W - 1 for W in k["windows"]), k["K"], k["K"])
        assert np.isfinite(k["cost64"]).all() and (k["bar"] > 0).all() and (k["bar"] < 1e-3 * np.maximum(k["cost64"], 1.0)).all()


def test_cost_is_symmetric_under_swapping_the_roles():
    F, hop, poses, trans, u, w, tw = _two_windows()
    K, O = 3, F - hop
    m = ref.cost(poses, trans, (2,), (21,), K, hop, u, w, tw)
    sp, st = poses.copy(), trans.copy()
    sp[:K, hop:], sp[K:, :O] = poses[K:, :O], poses[:K, hop:]
    st[:K, hop:], st[K:, :O] = trans[K:, :O], trans[:K, hop:]
    ms = ref.cost(sp, st, (2,), (21,), K, hop, u, w, tw)
    assert np.allclose(ms[0], m[0].T, rtol=1e-12, atol=0) and not np.allclose(m[0], m[0].T)


def test_cost_is_zero_for_identical_rows_and_tiny_for_aliases():
    F, hop, poses, trans, u, w, tw = _two_windows()
    K, O = 3, F - hop
    p = poses.copy()
    p[K:, :O] = p[:K, hop:]                                 # candidate c of the later window repeats candidate c of the earlier one
    m = ref.cost(p, None, (2,), (21,), K, hop, u, w, 0.0)
    # zero up to float64 rounding: conj(q) q in amuse_rot.hpp's association, (w y + x z) - y w - z x, leaves an angle of order 1e-16 rad, i.e. a cost below
    # 55 joints x 3 rows x (1e-15)^2; the neighbours' cost is of order 1
    assert (np.diag(m[0]) < 1e-27).all() and (m[0][~np.eye(K, dtype=bool)] > 1e-3).all()
    only_alias = np.where(np.arange(55) % sc.N_CLASSES == 4, 1.0, 0.0).astype(np.float32)
    ma = ref.cost(poses, None, (2,), (21,), K, hop, u, only_alias, 0.0)
    th = np.linalg.norm(poses[:K, hop:][:, :, np.arange(55) % sc.N_CLASSES == 4], axis=-1)
    assert ma.max() < 1e-9 and th.min() > 1e-3              # rotations of up to 3 rad and their aliases: the same rotations


def test_zero_weight_joints_do_not_move_the_cost():
    F, hop, poses, trans, u, w, tw = _two_windows()
    m = ref.cost(poses, trans, (2,), (21,), 3, hop, u, w, tw)
    p = poses.copy()
    p[:, :, w == 0] = sc.rand_aa(np.random.default_rng(5), p[:, :, w == 0].shape[:-1], 3.0)
    assert np.array_equal(ref.cost(p, trans, (2,), (21,), 3, hop, u, w, tw), m)
    p[:, :, 0] += 0.1
    assert not np.array_equal(ref.cost(p, trans, (2,), (21,), 3, hop, u, w, tw), m)


def _check_against_brute_force(windows, K, m):
    choice, total = ref.best_path(m, windows, K)
    s0 = g0 = 0
    for s, W in enumerate(windows):
        cands, tot = ref.brute_force(m, W, K, s0)
        assert [int(r) - (g0 + k) * K for k, r in enumerate(choice[g0:g0 + W])] == cands, (windows, K, s)
        assert total[s].tobytes() == np.float64(tot).tobytes()
        s0, g0 = s0 + W - 1, g0 + W


def test_dynamic_programme_is_brute_force_on_integer_matrices_with_ties():
    ties = 0
    for windows, K, m in sc.int_matrices():
        _check_against_brute_force(windows, K, m)
        for s, W in enumerate(windows):
            s0 = sum(w - 1 for w in windows[:s])
            _, tot = ref.brute_force(m, W, K, s0)
            ties += sum(ref.path_total(m, K, s0, p) == tot for p in itertools.product(range(K), repeat=W)) > 1
    assert ties >= 5                                         # the tie rule is really exercised


def test_dynamic_programme_is_brute_force_on_random_doubles():
    rng = np.random.default_rng(3)
    for windows, K in (((4,), 3), ((2, 1, 5), 2), ((6,), 3), ((3,), 5)):
        _check_against_brute_force(windows, K, rng.uniform(0, 10, (sum(W - 1 for W in windows), K, K)))


def test_non_finite_entries_never_win_and_all_non_finite_is_candidate_zero():
    m = np.array([[[np.nan, 5.0], [np.inf, -np.inf]], [[1.0, np.nan], [2.0, 0.5]]])
    choice, total = ref.best_path(m, (3,), 2)
    assert choice.tolist() == [0, 3, 5] and total[0] == 5.5                  # only a = 0 -> b = 1 is finite at the first seam
    choice, total = ref.best_path(np.full((2, 2, 2), np.nan), (3,), 2)
    assert choice.tolist() == [0, 2, 4] and np.isinf(total[0])
    choice, total = ref.best_path(np.zeros((0, 4, 4)), (1, 1), 4)
    assert choice.tolist() == [0, 4] and total.tolist() == [0.0, 0.0]


def test_select_is_a_row_gather():
    p = np.arange(6 * 2 * 55 * 3, dtype=np.float32).reshape(6, 2, 55, 3)
    po, to = ref.select(p, None, np.array([1, 2, 5]))
    assert to is None and np.array_equal(po, p[[1, 2, 5]])


def test_plan_numbers():
    assert ref.plan((3, 1), 2, 12, 9) == (2, 2 * 2 * 2 * 3 * 55 * 16) and ref.plan((1,), 4, 300, 270) == (0, 0)
    from amuse_amd import seam
    for windows, K, F, hop in (((3, 1), 2, 12, 9), ((1,), 4, 300, 270), ((40,), 64, 300, 270), ((3, 2, 4), 5, 300, 150)):
        p = seam.plan(windows, K, hop, F)
        assert (p["seams"], p["workspace_bytes"]) == ref.plan(windows, K, F, hop)
