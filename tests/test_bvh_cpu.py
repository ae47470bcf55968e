"""CPU: BVH export without a GPU - that the references and the inputs of tests/test_gpu_bvh.py are sound, and everything of the feature that needs no kernel:
the library's column order (amuse_bvh_layout) against a Python depth-first walk, the header and the reader on a synthetic body model, the float64 unwrap rule
on the crafted curves, the fp32 restatement against scipy, Python's "%11.6f" against the exactness argument the formatter rests on, the refusals."""
import ctypes as C

import numpy as np
import pytest

import body_cases as bc
import bvh_cases as cases
import bvh_ref as ref


def _model():
    from amuse_amd.body import BodyModel
    return BodyModel.from_dict(bc.make_model())


SMPLX_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]     # the public model's, from memory


def test_joint_names_agree_with_the_rest_of_the_project():
    from amuse_amd import bvh, smooth
    from amuse_amd.npz_writer import LOWER_BODY_JOINTS
    assert len(bvh.JOINT_NAMES) == 55
    assert [bvh.JOINT_NAMES[j] for j in LOWER_BODY_JOINTS] == ["left_hip", "right_hip", "left_knee", "right_knee", "left_ankle", "right_ankle", "left_foot", "right_foot"]
    hands = [bvh.JOINT_NAMES[j] for j in smooth.HAND_JOINTS]
    assert len(hands) == 30 and all(n.startswith("left_") and n[-1] in "123" for n in hands[:15]) and all(n.startswith("right_") for n in hands[15:])
    assert not any(n[-1] in "123" and "spine" not in n for n in bvh.JOINT_NAMES[:25])


def test_layout_against_a_python_walk():
    from amuse_amd import _lib, bvh
    for parents in (SMPLX_PARENTS, list(bc.make_model()["parents"]), [-1], [-1, 0, 0, 0], [-1] + list(range(54))):
        assert list(bvh.layout(parents)) == ref.dfs(parents)
    g = np.random.default_rng(3)
    p = [-1] + [int(g.integers(0, j)) for j in range(1, 200)]
    got = list(bvh.layout(p))
    assert got == ref.dfs(p) and sorted(got) == list(range(200))
    d = bvh.layout(SMPLX_PARENTS)
    assert list(d[:6]) == [0, 1, 4, 7, 10, 2] and d[-1] == 54                 # the left leg first, the right hand's last finger last
    lib, ip = _lib.load(), C.POINTER(C.c_int)
    out = (C.c_int * 4)()
    for bad in ([0, 0, 1], [-1, 1, 0], [-1, 0, 2], [-1, -1, 0]):
        assert lib.amuse_bvh_layout((C.c_int * 3)(*bad), 3, out) != 0, bad
    assert lib.amuse_bvh_layout(None, 3, out) != 0 and lib.amuse_bvh_layout((C.c_int * 1)(-1), 0, out) != 0
    with pytest.raises(_lib.AmuseHipError):
        bvh.layout([0, 0])


@pytest.mark.parametrize("order", ["ZYX", "XZY"])
def test_header_reader_round_trip_on_a_synthetic_model(tmp_path, order):
    from amuse_amd import bvh
    m = _model()
    betas = bc.make_betas(1)[0]
    J = bvh.rest_joints(m, betas)
    # the float64 twin at the zero pose states the same joints (its Rodrigues adds 1e-8 to the vector: 1e-7 of slack)
    import torch
    from amuse_amd.body import torch_forward
    Jt = torch_forward(m, betas[None], torch.zeros(1, 1, 55, 3))[0][0, 0].numpy()
    assert np.abs(Jt - J).max() < 1e-6
    scale, F = 100.0, 3
    g = np.random.default_rng(0)
    vals = g.uniform(-180, 180, (F, 168)).astype(np.float32)
    hdr = bvh.header_text(m.parents, J, F, 30.0, order, scale)
    meta = {"gender": "neutral", "betas": [float(b) for b in betas], "scale": scale, "order": order, "root_rest": [float(x) for x in J[0]], "mocap_frame_rate": 30.0}
    p = bvh.write_bvh(tmp_path / "x_motion.bvh", hdr, ref.fmt(vals), meta)
    assert not list(tmp_path.glob("*.part")) and p.read_bytes().startswith(b"HIERARCHY\nROOT pelvis\n{\n\tOFFSET 0.000000 0.000000 0.000000\n\tCHANNELS 6 Xposition")
    assert len(p.read_bytes()) == len(hdr) + F * 2016
    b = bvh.read_bvh(p)
    dfs = ref.dfs(m.parents)
    assert list(b["dfs"]) == dfs and b["names"] == [bvh.JOINT_NAMES[j] for j in dfs]             # the file lists its joints in column order
    assert list(b["parents"]) == list(m.parents) and b["order"] == order and b["frames"] == F and b["frame_time"] == 0.033333
    want = np.zeros((55, 3))
    want[1:] = (J[1:] - J[m.parents[1:]]) * scale
    assert np.array_equal(b["offsets"], np.round(want, 6) + 0.0) or np.abs(b["offsets"] - want).max() <= 0.5e-6 + 1e-12
    leaves = sorted(set(range(55)) - set(int(x) for x in m.parents[1:]))
    assert sorted(b["end_sites"]) == leaves and all(np.abs(b["end_sites"][j] - want[j] * 0.5).max() <= 0.5e-6 + 1e-12 for j in leaves)
    assert np.array_equal(b["channels"], np.array([float("%.6f" % x) for x in vals.reshape(-1)]).reshape(F, 168))
    assert b["meta"] == meta
    # what the reader refuses
    bad = tmp_path / "bad_motion.bvh"
    text = p.read_text()
    for edit, msg in ((lambda t: "# a comment\n" + t, "not a BVH"), (lambda t: t.replace("JOINT jaw", "JOINT chin"), "55 SMPL-X joints"),
                      (lambda t: t.replace("Frames: 3", "Frames: 4"), "numbers in the MOTION block"),
                      (lambda t: t.replace(f"CHANNELS 3 {order[0]}rotation {order[1]}rotation", f"CHANNELS 3 {order[1]}rotation {order[0]}rotation", 1), "channel orders")):
        bad.write_text(edit(text))
        with pytest.raises(ValueError, match=msg):
            bvh.read_bvh(bad)


@pytest.mark.parametrize("order", ref.ORDERS)
def test_reference_unwrap_returns_the_generating_curves(order):
    for case, jump in ((cases.spin(order), 340.0), (cases.fold(order), 180.0)):
        F = case["poses"].shape[0]
        principal = ref.euler_ref(case["poses"], order).reshape(F, 55, 3)
        steps = np.abs(np.diff(principal, axis=0))
        assert steps.max() > jump - 1.0                                        # the principal values jump: the case discriminates
        un = ref.unwrap(principal)
        assert np.abs(un - case["curves"]).max() <= 5e-4                       # (fp32 axis-angle inputs near pi: half of the GPU test's cap of 1e-3 degrees)
        assert np.abs(np.diff(un, axis=0)).max() <= 20.0 + 1e-3
        assert ref.geodesic(case["poses"], un.reshape(-1, 3), order).max() <= 1e-9        # the same rotations
    # on float64 inputs the rule returns the curves to rounding
    from scipy.spatial.transform import Rotation
    c = cases.fold(order)["curves"]
    pr = Rotation.from_euler(order, c.reshape(-1, 3), degrees=True).as_euler(order, degrees=True).reshape(c.shape)
    assert np.abs(ref.unwrap(pr) - c).max() <= 1e-9 and c[-1, 0, 1] == 120.0
    w = ref.unwrap(ref.euler_ref(cases.wind(order)["poses"], order).reshape(37, 55, 3))
    assert np.abs(w[7, :, 0]).min() > 1000.0 and np.abs(w - cases.wind(order)["curves"]).max() <= 1e-3


@pytest.mark.parametrize("order", ref.ORDERS)
def test_fp32_restatement_against_scipy(order):
    c = cases.euler_cases(order)
    assert c["aa"].shape == (2200, 3) and np.linalg.norm(c["aa"][c["cls"]["beyond_pi"]], axis=-1).min() > np.pi
    assert np.linalg.norm(c["aa"][c["cls"]["tiny"]], axis=-1).max() < 1e-3 and not c["aa"][c["cls"]["tiny"]][:20].any()
    for name in ("gimbal_exact", "gimbal_near"):
        assert np.abs(np.abs(c["ref"][c["cls"][name], 1]) - 90.0).max() <= (1e-3 if name == "gimbal_near" else 2e-2)      # (fp32 axis-angle: 'exact' to its rounding)
    assert c["away"][c["cls"]["random"]].mean() > 0.9 and not c["away"][c["cls"]["gimbal_near"]].any()
    print(f"{order}: fp32 restatement geodesic max {c['f32_geo']:.3e} rad; channel margin (4 x its worst, away from lock) {c['margin']:.3e} deg")
    assert c["f32_geo"] <= 2.5e-6                      # a quarter of the kernel's bar of 1e-5
    assert np.abs(c["f32"][:, 1]).max() <= 90.0 and np.abs(c["f32"][:, [0, 2]]).max() <= 180.0
    assert 0 < c["margin"] < 0.05


def test_python_format_is_the_exact_integer():
    """what the kernel's formatter rests on: double(x) * 1e6 is exact, so rint of it is the integer "%11.6f" prints"""
    from fractions import Fraction
    v = cases.format_values()
    text = ref.fmt(v, 168)
    assert len(text) == 12 * v.size and text[11::12].count(b"\n") == v.size // 168 and text[2015:2016] == b"\n"
    for x, i in zip(v[3000:4096], range(3000, 4096)):
        prod = float(x) * 1e6
        assert Fraction(prod) == Fraction(float(x)) * 1000000
        want = int(np.rint(prod))
        field = text[12 * i:12 * i + 11].decode()
        assert int(field.replace(".", "").replace("-", "")) == abs(want) and (field.strip()[0] == "-") == bool(np.signbit(x))
    assert ref.fmt(np.float32([-0.0, -4e-7, 999.99994]), 3) == b"  -0.000000   -0.000000  999.999939\n"
    assert ref.fmt(np.float32([0.0078125, 0.0234375]), 9) == b"   0.007812    0.023438 "           # ties go to the even digit


def test_refusals_without_a_gpu(tmp_path):
    from amuse_amd import _lib, bvh
    from amuse_amd import main as cli
    lib = _lib.load()
    buf = np.zeros(64, np.float32)
    fp = lambda off=0: C.c_void_p(buf.ctypes.data + off)
    one, dfs = (C.c_int * 1)(3), (C.c_int * 55)(*range(55))
    assert lib.amuse_bvh_format(fp(), 0, 168, fp(), fp(), None) != 0 and lib.amuse_bvh_format(fp(), 4, 0, fp(), fp(), None) != 0
    assert lib.amuse_bvh_format(None, 4, 168, fp(), fp(), None) != 0 and lib.amuse_bvh_format(fp(), 4, 168, fp(2), fp(), None) != 0 and b"aligned" in lib.amuse_last_error()
    mo = lambda poses=fp(), rr=fp(), S=1, fr=one, d=dfs, order=5, scale=100.0, e=fp(), t=fp(), st=fp(): lib.amuse_bvh_motion(poses, None, rr, S, fr, d, order,
                                                                                                                            C.c_float(scale), 0, e, t, st, None)
    bad_dfs = (C.c_int * 55)(*([0] + list(range(54))))
    for kw in (dict(S=0), dict(fr=None), dict(fr=(C.c_int * 1)(0)), dict(order=6), dict(order=-1), dict(d=bad_dfs), dict(d=None), dict(scale=0.0), dict(scale=float("nan")),
               dict(poses=None), dict(rr=None), dict(st=None), dict(e=None, t=None), dict(t=fp(2))):
        assert mo(**kw) != 0, kw
    de = lambda ch=fp(), order=0, scale=1.0, out=fp(): lib.amuse_bvh_decode(ch, 1, one, dfs, order, C.c_float(scale), fp(), out, fp(), None)
    assert de(ch=None) != 0 and de(order=7) != 0 and de(scale=-1.0) != 0 and de(out=None) != 0
    with pytest.raises(ValueError, match="order"):
        bvh.options("ZYZ")
    with pytest.raises(ValueError, match="scale"):
        bvh.options("ZYX", 0)
    assert bvh.options("zyx", 1, 1) == {"order": "ZYX", "scale": 1.0, "unwrap": True}
    assert bvh.bvh_path("a/scott_seq_0_AbC123_motion_smplx.npz").name == "scott_seq_0_AbC123_motion.bvh" and bvh.bvh_path("o.npz", tmp_path) == tmp_path / "o_motion.bvh"
    assert bvh.npz_path_of("a/x_motion.bvh").name == "x_from_bvh_motion_smplx.npz"
    # the command lines
    for argv, msg in ((["--fn", "infer_gesture", "--bvh-order", "XYZ"], "belong to --bvh"), (["--fn", "infer_gesture", "--bvh-scale", "1"], "belong to --bvh"),
                      (["--fn", "infer_gesture", "--bvh-unwrap"], "belong to --bvh"), (["--fn", "infer_gesture", "--bvh"], "--bvh needs --smplx-models"),
                      (["--fn", "train_gesture", "--bvh", "--smplx-models", str(tmp_path)], "--bvh belongs to"),
                      (["--fn", "infer_gesture", "--bvh", "--smplx-models", str(tmp_path)], "were not all found")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(argv)
    with pytest.raises(SystemExit):
        bvh.main(["x_motion_smplx.npz"])                                        # no --smplx-models
    with pytest.raises(SystemExit):
        bvh.main(["--to-npz", "x_motion.bvh", "--order", "XYZ"])
    with pytest.raises(SystemExit, match="does not exist"):
        bvh.main([str(tmp_path / "x_motion_smplx.npz"), "--smplx-models", str(tmp_path)])
