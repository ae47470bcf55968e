"""GPU: the preview video encoder (csrc/k_mjpeg.hip through amuse_amd/video.py) against tests/mjpeg_ref.py's restatement, and the AVI a preview run writes.

Bars, and where they come from.
  coefficients     equal to the float64 restatement's, except where the float64 F / t lies within 2e-3 of a half-integer: there fp32 may round to the
                   neighbour (never further) and the coefficient is left out of the exact comparison; at most 3 % of a case may be left out (a condition on
                   the cases, not a tolerance).  tests/test_mjpeg_cpu.py holds a float32 numpy restatement to the same conditions.
  bit stream       every frame's bytes equal the restatement's header + the restatement's entropy coding of the GPU's OWN coefficients + EOI: the entropy
                   coding is a pure function of the coefficients, so there is nothing to tolerate.
  reproducibility  the same frame gives the same bytes alone, first, in the middle and last in a batch, and on two runs.
  capacity         with out_capacity below the total: sizes, offsets and total are the full run's, the frames that fit equal the full run's, and the guard
                   bytes behind out_capacity are untouched.
  PIL              PIL's decode of the GPU's file against the source >= PIL's own encode (same tables, subsampling 0) - 0.5 dB: the reference is libjpeg at
                   identical quantisation; the margin covers its integer DCT and its rounding of Y Cb Cr before the transform."""
import functools
import io
import os
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import mjpeg_cases as mc
import mjpeg_ref as mr

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
DEV = "cuda:0"
WINDOW, SHARE = 2e-3, 0.03


@functools.lru_cache(maxsize=None)
def _gpu(name):
    """the GPU's answers for a case, computed once and shared: coef int16 [M, my, mx, 3, 64], files [bytes]"""
    from amuse_amd import video
    fr = mc.frames(name)
    enc = video.JpegEncoder(DEV, fr.shape[2], fr.shape[1], mc.quality(name))
    dev = torch.from_numpy(fr.copy()).to(DEV)
    coef = enc.coefficients(dev).cpu().numpy()
    files = enc.encode(dev)
    enc.close()
    coef.setflags(write=False)
    return {"coef": coef, "files": files}


@pytest.mark.parametrize("name", mc.NAMES)
def test_coefficients_against_float64(name):
    ref, got = mc.reference(name), _gpu(name)["coef"]
    assert got.shape == ref["coef"].shape
    left_out = mr.near_half(ref["quotients"], WINDOW)
    diff = np.abs(got.astype(int) - ref["coef"])
    print(f"{name}: {left_out.mean():.4%} left out, {(diff != 0).sum()} of {diff.size} coefficients differ, max {diff.max()}")
    assert (got[~left_out] == ref["coef"][~left_out]).all()
    assert diff.max() <= 1
    assert left_out.mean() <= SHARE


@pytest.mark.parametrize("name", mc.NAMES)
def test_bit_stream_is_the_restatements_coding_of_the_gpus_coefficients(name):
    g, fr, q = _gpu(name), mc.frames(name), mc.quality(name)
    assert len(g["files"]) == len(fr)
    for m in range(len(fr)):
        want = mr.encode_coefficients(g["coef"][m], fr.shape[2], fr.shape[1], q)
        assert g["files"][m] == want, (name, m, len(g["files"][m]), len(want))


def test_a_frame_gives_the_same_bytes_anywhere_in_any_batch():
    from amuse_amd import video
    a, b, c = mc.frames("noise_24x20_q90")[0], mc.frames("batch3_24x20_q90")[1], mc.frames("batch3_24x20_q90")[2]
    enc = video.JpegEncoder(DEV, 24, 20, 90)
    up = lambda *f: torch.from_numpy(np.stack(f)).to(DEV)
    alone = enc.encode(up(a))[0]
    assert enc.encode(up(a, b, c))[0] == alone and enc.encode(up(b, a, c))[1] == alone and enc.encode(up(c, b, a))[2] == alone
    big = up(*([b, c] * 150 + [a]))                      # 301 frames: more than one block of the frame scan
    out = enc.encode(big)
    assert out[300] == alone and out[0] == out[298] and out[1] == out[299] and enc.encode(big) == out
    assert alone == _gpu("noise_24x20_q90")["files"][0]
    enc.close()


def test_capacity_is_never_passed():
    from amuse_amd import video
    fr = mc.frames("batch3_24x20_q90")
    dev = torch.from_numpy(fr.copy()).to(DEV)
    enc = video.JpegEncoder(DEV, 24, 20, 90)
    full = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    off, sz, tot = (t.cpu().numpy() for t in enc.encode_into(dev, full))
    total = int(tot[0])
    assert off.tolist() == [0, int(sz[0]), int(sz[0] + sz[1])] and total == int(sz.sum()) < full.numel()
    want = full.cpu().numpy()
    assert [want[o:o + s].tobytes() for o, s in zip(off, sz)] == _gpu("batch3_24x20_q90")["files"] and not want[total:].any()
    # capacities: nothing; inside the first header; inside the first frame's scan; between frames; inside the last frame; one byte short; exact
    for cap in (0, 100, mr.HEADER_BYTES + 37, int(off[1]), int(off[2]) + 300, total - 1, total):
        out = torch.full((total + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
        o2, s2, t2 = (t.cpu().numpy() for t in enc.encode_into(dev, out, capacity=cap))
        got = out.cpu().numpy()
        assert (o2 == off).all() and (s2 == sz).all() and int(t2[0]) == total, cap
        assert (got[cap:] == 0xA5).all(), cap                                             # the guard behind out_capacity is untouched
        assert (got[:cap] == want[:cap]).all(), cap                                       # what fits is the full run's, frames that fit are complete
    # the wrapper: a batch whose files are larger than its raw RGB (noise at quality 100) takes the second call
    noisy = mc.frames("noise_16x8_q100")
    assert len(mc.reference("noise_16x8_q100")["files"][0]) > noisy[0].size
    enc2 = video.JpegEncoder(DEV, 16, 8, 100)
    assert enc2.encode(torch.from_numpy(noisy.copy()).to(DEV)) == _gpu("noise_16x8_q100")["files"]
    enc.close()
    enc2.close()


def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))


def _pil_own(rgb, quality):
    from PIL import Image
    tl, tc = mr.tables(quality)
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", qtables=[[int(x) for x in tl], [int(x) for x in tc]], subsampling=0)
    return _decode(b.getvalue())


@pytest.mark.parametrize("name", mc.NAMES)
def test_pil_decodes_the_gpus_files(name):
    pytest.importorskip("PIL.Image")
    for f, data in zip(mc.frames(name), _gpu(name)["files"]):
        got = _decode(data)
        assert got.shape == f.shape
        ours, pils = mr.psnr(got, f), mr.psnr(_pil_own(f, mc.quality(name)), f)
        print(f"{name}: GPU {ours:.2f} dB, PIL's own encode {pils:.2f} dB")
        assert ours >= pils - 0.5


# ------------------------------------------------------------------ end to end
def _models(directory):
    import body_cases as bc
    import render_cases as rc
    from amuse_amd import body
    directory.mkdir()
    m = body.BodyModel.from_dict(dict(bc.make_model(V=203), faces=rc.random_faces(203, 400)))
    for name in body.SMPLX_FILES.values():
        m.to_npz(directory / name)
    return directory


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def _check_avi_against_pngs(avi_bytes, frames_dir, n, size, quality):
    a = mr.walk_avi(avi_bytes)
    video_chunks = [avi_bytes[o:o + s] for cc, o, s in a["movi"] if cc == b"00dc"]
    assert len(video_chunks) == n
    for k, data in enumerate(video_chunks):
        src = _png(frames_dir / f"frame_{k:04d}.png")
        got = _decode(data)
        assert got.shape == (size[1], size[0], 3)
        assert mr.psnr(got, src) >= mr.psnr(_pil_own(src, quality), src) - 0.5, k
    return a


def test_previewer_writes_the_avi_and_leaves_the_pictures(tmp_path):
    pytest.importorskip("PIL.Image")
    import body_cases as bc
    from scipy.io import wavfile
    from amuse_amd import body, render
    # (the previewer's images are square: 64 x 64 here; the 64 x 48 frame of the renderer's model goes through the encoder in the case render_64x48_q90)
    models = body.load_models(_models(tmp_path / "models"))
    aa, trans, _ = bc.make_motion(N=1, F=12, seed=3)
    npz = tmp_path / "clip_motion_smplx.npz"
    np.savez(npz, poses=aa[0].reshape(12, -1), trans=trans[0], betas=np.zeros(10, np.float32), gender="neutral")
    pcm = np.random.default_rng(9).integers(-32768, 32768, 7000, dtype=np.int16)      # 0.4375 s at 16 kHz: a tail beyond the 12 frames' 6400 samples
    wavfile.write(str(tmp_path / "clip.wav"), 16000, pcm)

    plain = render.Previewer(models, DEV, 64, 5, frames=True)
    w0 = plain.preview(npz, tmp_path / "plain")
    plain.close()
    assert not list((tmp_path / "plain").rglob("*.avi"))
    pv = render.Previewer(models, DEV, 64, 5, frames=True, video=True, quality=90)
    w1 = pv.preview(npz, tmp_path / "video", wav=tmp_path / "clip.wav")
    pv.close()
    assert [p.name for p in w1[:-1]] == [p.name for p in w0] and w1[-1].name == "clip_preview.avi"
    for p, q in zip(w0, w1):
        assert p.read_bytes() == q.read_bytes()                                       # the sheet and every frame PNG: byte-identical
    data = w1[-1].read_bytes()
    a = _check_avi_against_pngs(data, tmp_path / "video" / "clip_preview", 12, (64, 64), 90)
    assert b"".join(data[o:o + s] for cc, o, s in a["movi"] if cc == b"01wb") == pcm.tobytes()
    mr.check_avi(data, [data[o:o + s] for cc, o, s in a["movi"] if cc == b"00dc"], 64, 64, 30, pcm[:, None], 16000)
    # video without frames: the sheet keeps its bytes, no frame directory
    pv = render.Previewer(models, DEV, 64, 5, video=True)
    w2 = pv.preview(npz, tmp_path / "video_only")
    pv.close()
    assert [p.name for p in w2] == ["clip_preview.png", "clip_preview.avi"] and w2[0].read_bytes() == w0[0].read_bytes()
    b = mr.walk_avi(w2[1].read_bytes())
    assert len(b["streams"]) == 1 and [cc for cc, _, _ in b["movi"]] == [b"00dc"] * 12                   # no waveform at hand: the video stream alone
    assert [w2[1].read_bytes()[o:o + s] for _, o, s in b["movi"]] == [data[o:o + s] for cc, o, s in a["movi"] if cc == b"00dc"]


def test_non_square_frames_through_renderer_encoder_and_avi(tmp_path):
    """60 x 44 - neither a multiple of 8 - from the renderer's rgb_out, still on the device, through the encoder into an AVI with audio and back through the
    walker and PIL (the previewer's own images are square)"""
    pytest.importorskip("PIL.Image")
    import render_cases as rc
    from amuse_amd import body, render, video
    W, H, F = 60, 44, 3
    c = rc.body_case(width=W, height=H, frames=F)
    eng = body.BodyEngine(DEV, c["model"])
    eng.set_subjects(c["betas"])
    v = eng.vertices(torch.from_numpy(c["aa"]).to(DEV), torch.from_numpy(c["trans"]).to(DEV))[0].contiguous()
    ren = render.Renderer(DEV, c["faces"], 203, W, H, 2)
    rgb = ren.render(v, c["cam"])
    enc = video.JpegEncoder(DEV, W, H, 90)
    jpegs = enc.encode(rgb)
    src = rgb.cpu().numpy()
    for r in (enc, ren, eng):
        r.close()
    pcm = np.random.default_rng(4).integers(-32768, 32768, (F * 16000 // 30 + 77, 2), dtype=np.int16)
    with video.AviWriter(tmp_path / "v.avi", W, H, 30, (pcm, 16000)) as w:
        for j in jpegs:
            w.write_frame(j)
    a = mr.check_avi((tmp_path / "v.avi").read_bytes(), jpegs, W, H, 30, pcm, 16000)
    assert len(np.unique(src.reshape(-1, 3), axis=0)) > 10
    for k, (cc, o, s) in enumerate(x for x in a["movi"] if x[0] == b"00dc"):
        got = _decode((tmp_path / "v.avi").read_bytes()[o:o + s])
        assert got.shape == (H, W, 3) and mr.psnr(got, src[k]) >= mr.psnr(_pil_own(src[k], 90), src[k]) - 0.5, k


def test_dataset_driven_edit_muxes_the_takes_ld_waveform(tmp_path):
    """trainer on an --eval-data dictionary: the take that holds ld_waveform gets clip 0 of it at 16 kHz, the take that does not gets the video stream alone"""
    import random
    from conftest import make_reference_tree
    from amuse_amd import body, render, video
    from amuse_amd import main as cli
    from amuse_amd import weights as wts
    from amuse_amd.infer_ldm import PretrainedLPDM_v1
    from amuse_amd.trainer import trainer
    config, _ = cli.load_config(make_reference_tree(tmp_path / "tree"), "edit_gesture", None)
    tp = config["TRAIN_PARAM"]
    tp["test"]["emotion_control_list"]["use"] = False
    tp["motion_extractor"]["metrics_only"] = False
    tp["test"]["style_transfer"] = {"use": True, "overwrite": None, "actors": "[scott-miranda]", "emotion": "[fear]"}
    wave = (0.5 * torch.sin(torch.arange(160000 + 3000) / 7.0))[None]                 # (1, n): one clip and a rest the clip does not take

    def take(k, actor, gender, **extra):      # precomputed latents (no ld_motion: nothing is embedded)
        g = torch.Generator().manual_seed(100 + k)
        con, emo, sty = (torch.randn(1, 256, generator=g) for _ in range(3))
        return dict({"ld_z": torch.zeros(1, 128), "ld_z_con": con, "ld_z_emo": emo, "ld_z_sty": sty, "ld_attr": (actor, gender, "native", "x", "30"),
                     "ld_wav": np.zeros(10000, np.float32)}, **extra)
    f1, f2 = "0_103_103", "0_104_104"      # 8 jobs: per take both originals, then both with the other actor's style; every job keeps its own take's content
    data = {"style_transfer_info": "[scott-miranda]_[fear]", "style_transfer": {
        "scott": {f1: take(2, "scott", "male", ld_emo_label="fear", ld_waveform=wave), f2: take(3, "scott", "male", ld_emo_label="fear", ld_waveform=wave)},
        "miranda": {f1: take(4, "miranda", "female", ld_emo_label="fear"), f2: take(5, "miranda", "female", ld_emo_label="fear")}}}
    m = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device=DEV, seed=2024)
    m.precision = "fp32x"
    m.set_sampler("ddim", 4)
    m.emotion_control, m.style_transfer, m.style_Xemo_transfer = False, True, False
    random.seed(5)
    tr = trainer(config, torch.device(DEV), train_loader=data, model_path=tmp_path / "saved", model=m, stamp="s")
    written = tr.eval_prior_latdiff_forward_backward_v1(False, 7, False, False, modelversion="full", ammetric=True)
    m.engine.close()
    assert len(written) == 8
    assert set(tr.preview_audio) == {str(p) for p in written if p.name.startswith("scott")} and len(tr.preview_audio) == 4
    assert all(e[0] == "ld_waveform" and e[1] is wave and e[2] == 0 for e in tr.preview_audio.values())
    scott, miranda = (next(p for p in written if p.name.startswith(a)) for a in ("scott", "miranda"))
    pv = render.Previewer(body.load_models(_models(tmp_path / "models")), DEV, 32, 100, video=True)
    try:
        out = {p: pv.preview(p, wav=video.preview_wav(tr.preview_audio.get(str(p)))) for p in (scott, miranda)}
    finally:
        pv.close()
    a = mr.walk_avi(out[scott][-1].read_bytes())
    want = np.clip(np.rint(wave[0, :160000].double().numpy() * 32768), -32768, 32767).astype("<i2").tobytes()
    data_s = out[scott][-1].read_bytes()
    assert len(a["streams"]) == 2 and b"".join(data_s[o:o + s] for cc, o, s in a["movi"] if cc == b"01wb") == want
    assert struct.unpack("<HHI", a["streams"][1][1][:8]) == (1, 1, 16000) and sum(cc == b"00dc" for cc, _, _ in a["movi"]) == 300
    b = mr.walk_avi(out[miranda][-1].read_bytes())
    assert len(b["streams"]) == 1 and [cc for cc, _, _ in b["movi"]] == [b"00dc"] * 300


def _run_cli(root, extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "AMUSE_RUN_STAMP")}
    env.update(AMUSE_RUN_STAMP="20260101-000000")
    r = subprocess.run([sys.executable, "-m", "amuse_amd.main", "--fn", "infer_gesture", "--root", str(root), "--random-init"] + extra,
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return sorted(p for p in root.rglob("*") if p.is_file() and p.suffix in (".npz", ".png", ".avi") and "viz_dump" in p.parts)


def test_cli_preview_video(tmp_path):
    pytest.importorskip("PIL.Image")
    from conftest import make_reference_tree
    from amuse_amd import video
    models = _models(tmp_path / "models")
    common = ["--preview", "--preview-frames", "--smplx-models", str(models), "--preview-size", "32", "--preview-stride", "50"]
    a = _run_cli(make_reference_tree(tmp_path / "a", n_infer_wavs=1), common)
    root = make_reference_tree(tmp_path / "b", n_infer_wavs=1)
    b = _run_cli(root, common + ["--preview-video"])
    assert not [p for p in a if p.suffix == ".avi"]                                   # off by default
    avis = [p for p in b if p.suffix == ".avi"]
    rest = [p for p in b if p.suffix != ".avi"]
    assert len(avis) == len([p for p in a if p.suffix == ".npz"]) >= 1
    assert [p.relative_to(tmp_path / "a") for p in a] == [p.relative_to(root) for p in rest]
    for p, q in zip(a, rest):
        assert p.read_bytes() == q.read_bytes(), p.name                               # every NPZ and PNG keeps its bytes
    wav = sorted((root / "viz_dump/test/speech").glob("*.wav"))
    assert len(wav) == 1
    pcm, rate = video.load_pcm16(wav[0])
    for avi in avis:
        F = int(np.load(avi.with_name(avi.name.replace("_preview.avi", "_motion_smplx.npz")))["poses"].shape[0])
        data = avi.read_bytes()
        w = _check_avi_against_pngs(data, avi.with_suffix(""), F, (32, 32), 90)
        assert b"".join(data[o:o + s] for cc, o, s in w["movi"] if cc == b"01wb") == pcm.tobytes()      # the audio is the WAV's
        assert w["streams"][1][1][:8] == np.array([1, pcm.shape[1]], "<u2").tobytes() + np.array([rate], "<u4").tobytes()
