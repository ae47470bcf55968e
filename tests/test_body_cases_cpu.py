"""CPU: known answers on the numpy restatement of the SMPL-X body model (tests/body_ref.py) - no `smplx` package exists to pin it against - and the distances
that set the GPU bars of tests/test_gpu_body.py (computed there again from each case's own inputs; here they are held to their order of magnitude)."""
import numpy as np

import body_cases as bc
import body_ref as br

MODEL, BETAS = bc.make_model(), bc.make_betas()
# a skinning row is normalised in float32: its sum is 1 within 55 x 2^-24, so "rigid" statements over blended rows hold to that times the coordinates (< 3 m)
WSUM = 3 * 55 * 2.0 ** -24


def test_fixture_shape():
    m = MODEL
    assert m["v_template"].shape == (203, 3) and m["shapedirs"].shape == (203, 3, 300) and m["posedirs"].shape == (486, 609)
    p = m["parents"]
    assert p[0] == -1 and all(0 <= p[j] < j for j in range(1, 55))
    depth = np.zeros(55, int)
    for j in range(1, 55):
        depth[j] = depth[p[j]] + 1
    assert depth.max() >= 11                                                 # SMPL-X's finger depth
    nnz = (m["weights"] != 0).sum(1)
    assert set(nnz[3:]) == {1, 2, 3, 4} and (nnz[:3] == 55).all()            # rows of 1..4 non-zeros plus fully dense rows
    a = np.abs(m["posedirs"])
    assert a.max() < 1.1e-2 and a.min() < 2e-7                               # realistic scale
    aa, _, _ = bc.make_motion(3, 5)
    ang = np.linalg.norm(aa, axis=-1)
    assert (ang == 0).any() and (ang > np.pi).any()


def test_zero_pose_is_the_shaped_template():
    N, F = 2, 3
    tr = np.random.default_rng(0).standard_normal((N, F, 3))
    j, v = br.forward(MODEL, BETAS[:N], np.zeros((N, F, 55, 3)), tr)
    vs, J = br.shape(MODEL, BETAS[:N])
    assert np.abs(v - (vs[:, None] + tr[:, :, None])).max() < WSUM
    assert np.abs(j - (J[:, None] + tr[:, :, None])).max() < 1e-12
    assert np.array_equal(br.rodrigues(np.zeros(3)), np.eye(3))              # a zero vector gives the identity


def test_global_rotation_is_rigid_about_the_pelvis():
    model = dict(MODEL, posedirs=MODEL["posedirs"] * 0)                      # (the pose blend shapes ignore joint 0: zeroed only to keep the statement exact)
    rot = np.zeros((1, 1, 55, 3))
    rot[0, 0, 0] = [0.3, -1.1, 2.9]                                          # angle 3.1: close to pi
    j, v = br.forward(model, BETAS[:1], rot)
    vs, J = br.shape(model, BETAS[:1])
    R = br.rodrigues(rot[0, 0, 0])
    assert np.abs(v[0, 0] - ((vs[0] - J[0, 0]) @ R.T + J[0, 0])).max() < WSUM
    assert np.abs(j[0, 0] - ((J[0] - J[0, 0]) @ R.T + J[0, 0])).max() < 1e-12
    j2, v2 = br.forward(MODEL, BETAS[:1], rot)                               # and with the blend shapes in place: pose_feature skips joint 0
    assert np.abs(v2 - v).max() < 1e-12


def test_one_hot_row_follows_its_joint():
    w = MODEL["weights"].copy()
    w[10] = 0
    w[10, 17] = 1.0
    model = dict(MODEL, weights=w)
    aa, tr, _ = bc.make_motion(1, 2)
    j, v = br.forward(model, BETAS[:1], aa, tr)
    vs, J = br.shape(model, BETAS[:1])
    R = br.rodrigues(aa.astype(np.float64))
    GR, Gt = br.chain(R, J[:, None], model["parents"])
    pf = (R[:, :, 1:] - np.eye(3)).reshape(2, 486)
    vp = vs[0, 10] + (pf @ model["posedirs"].astype(np.float64)).reshape(2, 203, 3)[:, 10]
    want = np.einsum("fab,fb->fa", GR[0, :, 17], vp - J[0, 17]) + Gt[0, :, 17] + tr[0]
    assert np.abs(v[0, :, 10] - want).max() < 1e-12


def test_axis_angle_and_6d_agree_and_loop_equals_einsum():
    aa, tr, d6 = bc.make_motion(2, 3)
    j, v = br.forward(MODEL, BETAS[:2], aa, tr)
    j6, v6 = br.forward(MODEL, BETAS[:2], d6, tr, "6d")
    assert np.abs(v6 - v).max() < 5e-7 and np.abs(j6 - j).max() < 5e-7       # the 6D values are float32 roundings of the rotation's rows
    R = br.rodrigues(aa.astype(np.float64))
    j6d, v6d = br.forward(MODEL, BETAS[:2], br.matrix_to_rot6d(R), tr, "6d")
    # (the published Rodrigues form divides by |r + 1e-8|, so its matrix is a rotation only to ~1e-8; the Gram-Schmidt of its rows is one exactly)
    assert np.abs(v6d - v).max() < 1e-7 and np.abs(j6d - j).max() < 1e-7
    jl, vl = br.forward_loop(MODEL, BETAS[:1], aa[:1, :2], tr[:1, :2])
    assert np.abs(vl - v[:1, :2]).max() < 1e-13 and np.abs(jl - j[:1, :2]).max() < 1e-13
    jl6, vl6 = br.forward_loop(MODEL, BETAS[:1], d6[:1, :1], tr[:1, :1], "6d")
    assert np.abs(vl6 - v6[:1, :1]).max() < 1e-13


def test_loss_fixture_reaches_both_branches():
    sets = bc.make_loss_sets(3, 5)
    v = [br.forward(MODEL, BETAS, s[0], s[1])[1] for s in sets]
    d = np.abs(v[1] - v[0])
    assert (d > 1).any() and (d < 1).any()
    s = br.loss_sums(MODEL, BETAS, *[(x[0], x[1]) for x in sets], "aa", frames_per_pass=2)
    assert abs(s[0] - br.smooth_l1_sum(v[1], v[0])) < 1e-9 * s[0] and abs(s[1] - br.smooth_l1_sum(v[2], v[0])) < 1e-9 * s[1]
    assert br.smooth_l1_sum([0.5, 3.0], [0.0, 0.0]) == 0.125 + 2.5


def test_bar_distances():
    """d32 / dx / d16 and the loss sums' relative distances for the standard case.  Decision recorded here: the packer pre-scales posedirs by a power of two -
    without it the split product's distance is the larger one (entries of 1e-7 lose their lo piece under fp16's smallest subnormal)."""
    aa, tr, _ = bc.make_motion(3, 17)
    _, v, d = bc.forward_distances(MODEL, BETAS, aa, tr)
    print({k: f"{x:.3e}" for k, x in d.items()})
    ulp = np.spacing(np.float32(np.abs(v).max()))
    assert ulp < d["d32"] < 8 * ulp                                          # float32's rounding class at this magnitude
    assert d["dx"] < 2 * d["d32"]                                            # the split product sits in the same class ...
    assert d["dx_noscale"] > d["dx"]                                         # ... only with the pre-scale
    assert 10 * d["d32"] < d["d16"] < 1e-4                                   # one product: fp16's 11 bits on offsets of ~1e-2
    assert br.posedirs_shift(MODEL["posedirs"]) == 20
    s64, r = bc.loss_distances(MODEL, BETAS, bc.make_loss_sets(3, 17))
    print(s64, {k: f"{x:.3e}" for k, x in r.items()})
    assert r["r32"] < 2.0 ** -20 and r["rx"] < 2.0 ** -20 and r["r16"] < 1e-5
