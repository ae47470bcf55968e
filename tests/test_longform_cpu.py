"""CPU: long-form inference without a GPU - the window plan (the library's, against known answers and tests/stitch_ref.py's restatement), the refusals of both
entry points (made before any HIP call), the restatement's own known answers (it is the GPU tests' reference), the NPZ writer at 750 frames, the job list of
the trainer (header-only sample counts, one job per WAV, a WAV's windows on one rank) and the command line's switches."""
import ctypes as C

import numpy as np
import pytest
import torch

import stitch_ref as sr
from amuse_amd import _lib, longform

HOPS = (150, 180, 270, 300)


def test_plan_known_answers():
    for (n, h), (W, L) in {(160000, 270): (1, 300), (160534, 270): (2, 301), (400000, 270): (3, 750), (400000, 300): (3, 750), (0, 270): (1, 300)}.items():
        p = longform.plan(n, h)
        assert (p["windows"], p["frames"], p["hop_samples"]) == (W, L, h // 3 * 1600), (n, h, p)
        assert sr.plan(n, h) == (W, L, h // 3 * 1600)
    assert longform.plan(400000)["windows"] == 3 and longform.DEFAULT_HOP == 270           # the product's default hop
    assert longform.window_slices(400000, 270) == [(0, 160000), (144000, 304000), (288000, 400000)]
    assert longform.window_slices(1000, 270) == [(0, 1000)] and longform.window_slices(0, 270) == [(0, 0)]


def test_plan_matches_restatement_and_last_window_holds_audio():
    lib = _lib.load()
    W, L, hs = C.c_int(), C.c_int(), C.c_int()
    for h in HOPS:
        for n in range(0, 1000001, 533):
            assert lib.amuse_longform_plan(n, h, C.byref(W), C.byref(L), C.byref(hs)) == 0
            assert (W.value, L.value, hs.value) == sr.plan(n, h), (n, h)
            # what the join asks of (W, L), and the header's bound: the last window of a cut waveform holds more than 300 - h frames of audio
            assert (W.value - 1) * h < L.value <= (W.value - 1) * h + 300
            if W.value > 1:
                assert (n - (W.value - 1) * hs.value) * 3 > (300 - h) * 1600, (n, h)
            if n <= 160000:
                assert (W.value, L.value) == (1, 300)
    sl = longform.window_slices(999999, 180)
    assert sl == sr.window_slices(999999, 180) and sl[-1][1] == 999999 and all(b - a == 160000 for a, b in sl[:-1]) and 0 < sl[-1][1] - sl[-1][0] <= 160000


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.amuse_last_error().decode()
    for h in (271, 147, 303):
        assert lib.amuse_longform_plan(400000, h, None, None, None) == -1 and "hop_frames" in err()
        with pytest.raises(_lib.AmuseHipError):
            longform.plan(400000, h)
    assert lib.amuse_longform_plan(-1, 270, None, None, None) == -1 and "negative" in err()
    one = 0x1000                                           # (a non-null address that is never dereferenced: every call below fails in its checks)
    ints = lambda *v: (C.c_int * len(v))(*v)
    call = lambda S, W, L, F, hop, poses=one, trans=one, blend=one, po=one, to=one: lib.amuse_stitch_windows(poses, trans, S, W, L, F, hop, blend, po, to, None)
    assert call(0, ints(3), ints(30), 12, 9) == -1 and "S 0" in err()
    assert call(1, ints(3), ints(30), 1, 1) == -1 and "F 1" in err()
    assert call(1, ints(3), ints(30), 12, 5) == -1 and "hop 5" in err()          # more than two windows would cover a frame
    assert call(1, ints(3), ints(30), 12, 13) == -1 and "hop 13" in err()
    assert call(1, ints(0), ints(12), 12, 9) == -1 and "0 windows" in err()
    assert call(2, ints(3, 1), ints(18, 12), 12, 9) == -1 and "sequence 0" in err()   # L == (W - 1) hop: an empty last window
    assert call(2, ints(3, 1), ints(31, 12), 12, 9) == -1 and "sequence 0" in err()   # a frame no window produced
    assert call(2, ints(3, 1), ints(30, 13), 12, 9) == -1 and "sequence 1" in err()
    assert call(1, None, ints(30), 12, 9) == -1 and call(1, ints(3), None, 12, 9) == -1
    assert call(1, ints(3), ints(30), 12, 9, poses=None) == -1 and call(1, ints(3), ints(30), 12, 9, po=None) == -1
    assert call(1, ints(3), ints(30), 12, 9, blend=None) == -1 and "blend" in err()
    assert call(1, ints(3), ints(30), 12, 9, trans=None) == -1 and "together" in err()
    assert call(1, ints(3), ints(30), 12, 9, to=None) == -1
    with pytest.raises(_lib.AmuseHipError, match="no CPU fallback"):
        longform.stitch(torch.zeros(1, 300, 55, 3), None, [1], [300], 270)


def test_blend_weights():
    for O in (0, 1, 3, 30, 150):
        w = longform.blend_weights(O)
        assert w.dtype == torch.float32 and w.shape == (O,) and np.array_equal(w.numpy(), sr.blend_weights(O))
        if O:
            assert 0 < float(w[0]) and float(w[-1]) < 1 and bool((w[1:] > w[:-1]).all())
            assert np.abs(w.numpy().astype(np.float64) + w.numpy()[::-1] - 1).max() < 1e-7           # symmetric about the overlap's middle
    assert abs(float(longform.blend_weights(1)[0]) - 0.5) < 1e-7 and abs(float(longform.blend_weights(3)[0]) - (0.5 - 0.5 * np.cos(np.pi / 4))) < 1e-7


def test_restatement_known_answers():
    ax = np.array([0.6, -0.48, 0.64])                      # a unit axis
    got = sr.blend_joints(0.2 * ax, 0.6 * ax, 0.25)        # same axis: the angle interpolates linearly
    assert np.abs(got - 0.3 * ax).max() < 1e-14
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((50, 3)), rng.standard_normal((50, 3))
    assert sr.geodesic(sr.blend_joints(a, b, 1e-12), a).max() < 1e-10 and sr.geodesic(sr.blend_joints(a, b, 1 - 1e-12), b).max() < 1e-10   # the ends
    assert sr.geodesic(sr.blend_joints(a, b, 0.0), a).max() < 1e-14 and sr.geodesic(sr.blend_joints(a, b, 1.0), b).max() < 1e-14
    # a and its 2 pi - theta alias (the same rotation written the long way round) blend to the same rotation, and the result is the short form
    th = np.linalg.norm(a, axis=-1, keepdims=True)
    alias = -(a / th) * (2 * np.pi - th)
    assert sr.geodesic(a, alias).max() < 1e-12
    r1, r2 = sr.blend_joints(a, b, 0.3), sr.blend_joints(alias, b, 0.3)
    assert sr.geodesic(r1, r2).max() < 1e-12 and np.linalg.norm(r2, axis=-1).max() <= np.pi + 1e-12
    assert sr.geodesic(sr.blend_joints(b, alias, 0.6), sr.blend_joints(b, a, 0.6)).max() < 1e-12
    # halfway between two rotations about one axis by angles whose difference passes pi: the SHORTER arc
    assert np.abs(sr.blend_joints(np.array([0, 0, 3.0]), np.array([0, 0, -3.0]), 0.5) - np.array([0, 0, np.pi])).max() < 1e-12
    # tiny and equal inputs: no division by a vanishing sine
    assert np.abs(sr.blend_joints(np.zeros(3), np.zeros(3), 0.4)).max() == 0 and np.abs(sr.blend_joints(a, a, 0.7) - sr.quat_to_aa(sr.aa_to_quat(a))).max() < 1e-15
    assert np.abs(sr.blend_joints(1e-9 * ax, 3e-9 * ax, 0.5) - 2e-9 * ax).max() < 1e-20
    # the float32 restatement stays near the float64 one (what the GPU bars are built on)
    d = sr.geodesic(sr.blend_joints(a.astype(np.float32), b.astype(np.float32), 0.3, np.float32), sr.blend_joints(a.astype(np.float32), b.astype(np.float32), 0.3))
    assert d.max() < 2e-6


def test_restatement_join_copies_and_lerps():
    rng = np.random.default_rng(1)
    F, hop, W, L = 12, 9, 3, 28
    poses, trans = rng.standard_normal((W + 1, F, 55, 3)).astype(np.float32), rng.standard_normal((W + 1, F, 3)).astype(np.float32)
    blend = sr.blend_weights(F - hop)
    po, to, mask = sr.join(poses, trans, [W, 1], [L, F], hop, blend)
    assert po.shape == (L + F, 55, 3) and to.shape == (L + F, 3) and po.dtype == np.float64
    assert mask.nonzero()[0].tolist() == [9, 10, 11, 18, 19, 20]                               # frames two windows produced
    for f in range(L):
        k = min(f // hop, W - 1)
        if not mask[f]:
            assert np.array_equal(po[f], poses[k, f - k * hop]) and np.array_equal(to[f], trans[k, f - k * hop]), f       # copies
        else:
            w = np.float64(blend[f - k * hop])
            assert np.array_equal(to[f], (1 - w) * trans[k - 1, f - (k - 1) * hop].astype(np.float64) + w * trans[k, f - k * hop])    # the lerp
            assert sr.geodesic(po[f], sr.blend_joints(poses[k - 1, f - (k - 1) * hop], poses[k, f - k * hop], w)).max() == 0
    assert np.array_equal(po[L:], poses[W]) and not mask[L:].any()                             # the one-window sequence: all copies
    p2, t2, m2 = sr.join(poses[:3], None, [3], [36], 12, sr.blend_weights(0))                  # hop == F: concatenation
    assert t2 is None and not m2.any() and np.array_equal(p2, poses[:3].reshape(36, 55, 3))


def test_npz_fields_take_750_frames(tmp_path):
    from amuse_amd import npz_writer
    rng = np.random.default_rng(2)
    feat = rng.standard_normal((750, 168)).astype(np.float32)
    d = npz_writer.smplx_npz_fields(feat)
    assert d["poses"].shape == (750, 55, 3) and d["trans"].shape == (750, 3) and not d["trans"].any()
    low = npz_writer.LOWER_BODY_JOINTS
    assert np.array_equal(d["poses"][:, low], np.broadcast_to(feat[0, :165].reshape(55, 3)[low], (750, 8, 3)))   # the reference's freeze to frame 0
    up = [j for j in range(55) if j not in low]
    assert np.array_equal(d["poses"][:, up], feat[:, :165].reshape(750, 55, 3)[:, up])
    paths = npz_writer.write_sample(torch.from_numpy(feat)[None], tmp_path, "scott")
    assert len(paths) == 1
    with np.load(paths[0]) as z:
        assert z["poses"].shape == (750, 55, 3) and z["trans"].shape == (750, 3) and np.array_equal(z["poses"], d["poses"])


def _wavs(root, lengths):
    from scipy.io import wavfile
    rng = np.random.default_rng(3)
    d = root / "viz_dump/test/speech"
    for p in d.glob("*.wav"):
        p.unlink()
    for k, n in enumerate(lengths):
        wavfile.write(d / f"scott_0_{k}_{k}.wav", 16000, (rng.standard_normal(n) * 3000).astype(np.int16))
    return sorted(d.glob("*.wav"))


def test_wav_samples_reads_the_header_only(tmp_path):
    from scipy.io import wavfile
    from amuse_amd.trainer import load_wav, wav_samples
    rng = np.random.default_rng(4)
    cases = {"mono16": (rng.standard_normal(12345) * 3000).astype(np.int16), "stereo16": (rng.standard_normal((777, 2)) * 3000).astype(np.int16),
             "f32": rng.standard_normal(4001).astype(np.float32), "i32": (rng.standard_normal(31) * 1e6).astype(np.int32), "u8": rng.integers(0, 255, 999).astype(np.uint8)}
    for name, x in cases.items():
        wavfile.write(tmp_path / f"{name}.wav", 16000, x)
        assert wav_samples(tmp_path / f"{name}.wav") == x.shape[0] == load_wav(tmp_path / f"{name}.wav").shape[1], name
    (tmp_path / "bad.wav").write_bytes(b"not a wave file at all")
    with pytest.raises(ValueError, match="RIFF"):
        wav_samples(tmp_path / "bad.wav")


class _StubModel:
    """process_seq_list alone: an embedding that names its chunk (length, first sample), so the test can tell which windows were embedded"""
    device = "cpu"

    def __init__(self):
        self.seen = []

    def process_seq_list(self, chunks, framerate=16000, baseline=False):
        self.seen += [tuple(c.shape) for c in chunks]
        return [tuple(torch.full((1, 256), float(c.shape[1] + i)) for i in range(3)) for c in chunks]


def test_windows_of_one_wav_stay_on_one_rank(tmp_path):
    from conftest import make_reference_tree
    from amuse_amd import main as cli
    from amuse_amd.trainer import trainer
    root = make_reference_tree(tmp_path / "tree")
    lengths = [400000, 159744, 160534, 1000000, 16000, 700000]              # W = 3, 1, 2, 7, 1, 5 at hop 270
    audios = _wavs(root, lengths)
    config, _ = cli.load_config(root, "infer_gesture", None)
    config["TRAIN_PARAM"]["test"].update(long_form=True, hop_frames=270)
    want_W = [longform.plan(n, 270)["windows"] for n in lengths]
    assert want_W == [3, 1, 2, 7, 1, 5]
    owners = np.zeros(len(lengths), int)
    for rank in range(2):
        model = _StubModel()
        tr = trainer(config, "cpu", model=model, rank=rank, world=2)
        jobs, mine = tr._long_form_jobs(audios)
        assert [j["bsz"] for j in jobs] == want_W and [j["long_form"]["frames"] for j in jobs] == [longform.plan(n, 270)["frames"] for n in lengths]
        assert all(j["long_form"]["hop"] == 270 for j in jobs)
        for k, (j, m) in enumerate(zip(jobs, mine)):
            assert j["remote"] == (not m)
            if m:
                owners[k] += 1
                assert j["z_con"].shape == (want_W[k], 256) and j["z_emo"].shape == j["z_sty"].shape == (want_W[k], 256)
                # the windows of THIS waveform, in window order: full windows, then the short last one
                sl = longform.window_slices(lengths[k], 270)
                assert j["z_con"][:, 0].tolist() == [float(b - a) for a, b in sl] and j["z_sty"][:, 0].tolist() == [float(b - a) + 2 for a, b in sl]
        # only this rank's waveforms went through the front-end, whole: every window of a WAV is embedded where its job is sampled
        assert len(model.seen) == sum(w for w, m in zip(want_W, mine) if m) and all(s[0] == 1 for s in model.seen)
        # and the ranks' shares are contiguous job ranges (names and tags then follow the single-process order)
        idx = [k for k, m in enumerate(mine) if m]
        assert idx == list(range(idx[0], idx[-1] + 1))
    assert owners.tolist() == [1] * len(lengths)                           # every WAV on exactly one rank
    # one rank: everything local, and a short WAV's job is the default path's job (one window holding the whole waveform)
    model = _StubModel()
    jobs, mine = trainer(config, "cpu", model=model, rank=0, world=1)._long_form_jobs(audios)
    assert all(mine) and model.seen[3] == (1, 159744) and jobs[1]["bsz"] == 1 and jobs[1]["long_form"]["frames"] == 300


def test_cli_long_form_switches(tmp_path):
    from conftest import make_reference_tree
    from amuse_amd import main as cli
    root = make_reference_tree(tmp_path / "tree")
    for fn in ("edit_gesture", "train_gesture"):
        with pytest.raises(SystemExit, match="--long-form belongs to --fn infer_gesture"):
            cli.main(["--fn", fn, "--root", str(root), "--long-form"])
    for h in ("271", "147", "303"):
        with pytest.raises(SystemExit, match="--hop-frames"):
            cli.main(["--fn", "infer_gesture", "--root", str(root), "--long-form", "--hop-frames", h])
