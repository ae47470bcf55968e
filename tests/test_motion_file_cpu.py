"""CPU: amuse_amd/motion_file.py - the one reader of *_motion_smplx.npz, the sibling-name rule and the atomic writer - and body.fit_betas.  The modules that
use them keep their own path and file tests (test_bvh_cpu, test_render_cpu, test_smooth_cpu)."""
import numpy as np
import pytest
import torch

from amuse_amd import body, motion_file, npz_writer


def test_read_what_write_sample_wrote(tmp_path):
    feats = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 3, 168)).astype(np.float32))
    (p,) = npz_writer.write_sample(feats, tmp_path, "scott")
    m = motion_file.read(p)
    assert m.poses.shape == (3, 55, 3) and m.poses.dtype == np.float32 and m.trans.shape == (3, 3) and m.trans.dtype == np.float32
    assert m.betas.shape == (300,) and m.betas.dtype == np.float64 and isinstance(m.gender, str) and isinstance(m.fps, float) and m.path == p
    with np.load(p) as z:
        assert np.array_equal(m.poses, z["poses"]) and np.array_equal(m.trans, z["trans"].astype(np.float32)) and np.array_equal(m.betas, z["betas"])
        assert m.gender == str(z["gender"]) == "male" and m.fps == float(z["mocap_frame_rate"]) == 30.0
    assert np.array_equal(m.betas, npz_writer.fetchbetas("scott")) and m.betas.any()


def test_read_defaults_and_refusals(tmp_path):
    poses = np.random.default_rng(1).standard_normal((3, 165))
    np.savez(tmp_path / "only_poses.npz", poses=poses)
    m = motion_file.read(tmp_path / "only_poses.npz")
    assert np.array_equal(m.poses, poses.astype(np.float32).reshape(3, 55, 3))
    assert m.trans.shape == (3, 3) and m.trans.dtype == np.float32 and not m.trans.any()
    assert m.gender == "neutral" and m.betas.shape == (300,) and m.betas.dtype == np.float64 and not m.betas.any() and m.fps == 30.0
    np.savez(tmp_path / "j54.npz", poses=np.zeros((3, 54, 3), np.float32))
    with pytest.raises(ValueError, match="3 frames of 54 joints, not SMPL-X's 55"):
        motion_file.read(tmp_path / "j54.npz")
    np.savez(tmp_path / "f0.npz", poses=np.zeros((0, 55, 3), np.float32))
    with pytest.raises(ValueError, match="0 frames"):
        motion_file.read(tmp_path / "f0.npz")


def test_sibling(tmp_path):
    assert motion_file.sibling(tmp_path / "seq_0" / "x_motion_smplx.npz", "_preview.png") == tmp_path / "seq_0" / "x_preview.png"
    assert motion_file.sibling("other.npz", "_motion.bvh").as_posix() == "other_motion.bvh"
    assert motion_file.sibling("d/x_motion_smplx.npz", "_smoothed_motion_smplx.npz", tmp_path) == tmp_path / "x_smoothed_motion_smplx.npz"
    assert motion_file.sibling("d/x_motion.bvh", "_from_bvh_motion_smplx.npz", strip="_motion.bvh").as_posix() == "d/x_from_bvh_motion_smplx.npz"
    assert motion_file.sibling("a.b_motion_smplx.npz.bak", ".txt").name == "a.b_motion_smplx.npz.txt"      # no match: the stem, one suffix off


def test_atomic_replaces_under_an_open_reader(tmp_path):
    dst = tmp_path / "made" / "here" / "a_motion_smplx.npz"
    motion_file.save(dst, poses=np.zeros((2, 165), np.float32))
    old = open(dst, "rb")
    first = old.read(16)
    with motion_file.atomic(dst) as fh:
        assert dst.with_name(dst.name + ".part").exists() and open(dst, "rb").read(16) == first      # until the block ends the old file is the file
        fh.write(b"new bytes")
    old.seek(0)
    with np.load(old) as z:                                 # the handle on the replaced file still reads that file, whole
        assert z["poses"].shape == (2, 165)
    old.close()
    assert dst.read_bytes() == b"new bytes" and [p.name for p in dst.parent.iterdir()] == [dst.name]
    with pytest.raises(RuntimeError):                       # a block that fails replaces nothing
        with motion_file.atomic(dst) as fh:
            fh.write(b"half")
            raise RuntimeError
    assert dst.read_bytes() == b"new bytes"


@pytest.mark.parametrize("size", [9, 10, 11])
def test_fit_betas_is_the_pad_it_replaces(size):
    n = 10
    b64 = np.random.default_rng(size).standard_normal(size)
    b = b64.astype(np.float32)
    want = np.pad(b[:n], (0, max(0, n - b.size)))
    for got in (body.fit_betas(b, n), body.fit_betas(b64, n), body.fit_betas(b64[None], n)):
        assert got.dtype == np.float32 and got.shape == (n,) and got.tobytes() == want.tobytes()
