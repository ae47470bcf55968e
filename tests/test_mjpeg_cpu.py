"""CPU: the preview video encoder's host half and its restatement (tests/mjpeg_ref.py, tests/mjpeg_cases.py); amuse_amd/video.py's AVI writer; the command lines'
refusals.  No GPU: the kernels are held to the restatement in tests/test_gpu_mjpeg.py, the restatement is held to libjpeg (through PIL) here.

Bars, and where they come from.
  tables, header, plan   equal to the restatement / the arithmetic written out again: integers, nothing to tolerate.
  coefficients (fp32)    a float32 numpy restatement against the float64 one, under the two conditions tests/test_gpu_mjpeg.py sets for the kernel: a
                         coefficient whose float64 F / t lies within 2e-3 of a half-integer may differ by 1 and is left out; every other one is equal; at most
                         3 % per case are left out.  This shows the bar is reachable in fp32 before a GPU sees it.
  flat frames, q 100     decode to within 1 level: the only losses are one rounding of DC and the decoder's colour conversion.
  PSNR                   PIL's decode of the restatement's file against the source >= PIL's own encode (same tables, subsampling 0) - 0.5 dB: the reference is
                         libjpeg at identical quantisation; the margin covers its integer DCT and its rounding of Y Cb Cr before the transform."""
import ctypes as C
import io
import struct

import numpy as np
import pytest

import mjpeg_cases as mc
import mjpeg_ref as mr
from amuse_amd import _lib, video

WINDOW, SHARE = 2e-3, 0.03


def test_committed_tables_equal_pils():
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(mc.noise(16, 16, 1)).save(b, "JPEG", quality=50, subsampling=0)
    data, p, dht = b.getvalue(), 2, {}
    while data[p + 1] != 0xDA:
        n = struct.unpack(">H", data[p + 2:p + 4])[0]
        seg = data[p + 4:p + 2 + n]
        while data[p + 1] == 0xC4 and seg:
            k = sum(seg[1:17])
            dht[seg[0]] = (list(seg[1:17]), list(seg[17:17 + k]))
            seg = seg[17 + k:]
        p += 2 + n
    assert dht == {k: (list(b_), list(v)) for k, (b_, v) in mr.HUFFMAN.items()}
    q = Image.open(io.BytesIO(data)).quantization          # PIL at quality 50 writes the Annex K base tables
    assert list(q[0][:12]) == [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19], "PIL reports another order than natural: anchor on the rows"
    assert list(q[0]) == list(mr.BASE_LUMA) and list(q[1]) == list(mr.BASE_CHROMA)
    assert list(mr.BASE_CHROMA[:8]) == [17, 18, 24, 47, 99, 99, 99, 99]


def test_library_tables_equal_the_restatement_for_every_quality():
    for q in range(1, 101):
        lu, ch = video.tables(q)
        rl, rc = mr.tables(q)
        assert (lu == rl).all() and (ch == rc).all(), q
    assert (video.tables(50)[0] == mr.BASE_LUMA).all() and video.tables(100)[0].max() == 1 and video.tables(1)[1].min() == 255


def test_library_header_equals_the_restatement():
    for (w, h, q) in [(16, 8, 50), (24, 20, 90), (21, 19, 100), (512, 512, 90), (4096, 1, 1), (1, 4096, 75)]:
        assert video.header(w, h, q) == mr.header(w, h, q), (w, h, q)
    assert video.plan(512, 512, 1)["header_bytes"] == len(mr.header(512, 512, 90)) == mr.HEADER_BYTES
    codes = mr.CODES[0x10]
    assert codes[0x00] == (0b1010, 4) and codes[0xF0] == (0b11111111001, 11) and mr.CODES[0x00][0] == (0b00, 2)      # Annex K.3 known answers: EOB, ZRL, DC 0


def test_plan_known_answers_and_refusals():
    p = video.plan(512, 512, 300)
    assert (p["mcus_x"], p["mcus_y"], p["header_bytes"]) == (64, 64, 629)
    assert p["workspace_bytes"] == 300 * 4096 * 384 + 2 * 76800 + 1280
    assert p["worst_case_bytes_per_frame"] == 629 + 64 * 2 * (64 * 3 * 1660 // 8) + 2 * 63 + 2 == 5100277
    for (w, h, f) in [(16, 8, 1), (21, 19, 3), (40, 72, 7), (4096, 4096, 1), (1, 1, 1), (513, 7, 1800)]:
        assert video.plan(w, h, f) == mr.plan(w, h, f), (w, h, f)
    lib = _lib.load()
    assert lib.amuse_mjpeg_plan(8, 8, 1, None, None, None, None, None) == 0                 # every output is optional
    for (w, h, f) in [(0, 8, 1), (8, 0, 1), (4097, 8, 1), (8, 4097, 1), (-1, 8, 1), (8, 8, 0), (8, 8, -3), (4096, 4096, 2 ** 31 - 1)]:
        with pytest.raises(_lib.AmuseHipError):
            video.plan(w, h, f)
    for q in (0, 101, -5):
        with pytest.raises(_lib.AmuseHipError):
            video.tables(q)
        with pytest.raises(_lib.AmuseHipError):
            video.header(8, 8, q)
    lu = (C.c_ubyte * 64)()
    assert lib.amuse_mjpeg_tables(50, None, lu) != 0 and lib.amuse_mjpeg_tables(50, lu, None) != 0
    # every refusal of the calls comes before a HIP call (this machine has no GPU: a HIP call would fail with another code)
    EINVAL = lib.amuse_mjpeg_tables(0, lu, lu)
    assert lib.amuse_mjpeg_create(0, 0, 8, 90) is None and lib.amuse_mjpeg_create(0, 8, 4097, 90) is None and lib.amuse_mjpeg_create(0, 8, 8, 0) is None
    assert lib.amuse_mjpeg_create(0, 8, 8, 101) is None
    assert lib.amuse_mjpeg_reserve(None, 1) == EINVAL
    assert lib.amuse_mjpeg_encode(None, 1, 1, 1, 1, 1, 1, 1, None) == EINVAL
    assert lib.amuse_debug_mjpeg_coefficients(None, 1, 1, 1, None) == EINVAL
    lib.amuse_mjpeg_destroy(None)


@pytest.mark.parametrize("name", mc.NAMES)
def test_case_exercises_its_branch(name):
    mc.check_exercises_its_branch(name)


@pytest.mark.parametrize("name", mc.NAMES)
def test_float32_restatement_reaches_the_coefficient_bar(name):
    ref = mc.reference(name)
    for m, f in enumerate(mc.frames(name)):
        got = mr.quantise(mr.quotients(f, mc.quality(name), np.float32).astype(np.float64))
        left_out = mr.near_half(ref["quotients"][m], WINDOW)
        print(f"{name}[{m}]: {left_out.mean():.4%} left out, {(got != ref['coef'][m]).sum()} differ in all")
        assert (got[~left_out] == ref["coef"][m][~left_out]).all()
        assert np.abs(got.astype(int) - ref["coef"][m]).max() <= 1
        assert left_out.mean() <= SHARE


def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


@pytest.mark.parametrize("name", mc.NAMES)
def test_restatement_files_open_in_pil_and_hold_the_psnr_bar(name):
    Image = pytest.importorskip("PIL.Image")
    q = mc.quality(name)
    tl, tc = mr.tables(q)
    for f, data in zip(mc.frames(name), mc.reference(name)["files"]):
        im = _decode(data)
        assert im.size == (f.shape[1], f.shape[0]) and im.mode == "RGB" and im.format == "JPEG"
        assert list(im.quantization[0]) == list(tl) and list(im.quantization[1]) == list(tc)
        b = io.BytesIO()
        Image.fromarray(f).save(b, "JPEG", qtables=[[int(x) for x in tl], [int(x) for x in tc]], subsampling=0)
        ours, pils = mr.psnr(np.asarray(im), f), mr.psnr(np.asarray(_decode(b.getvalue())), f)
        print(f"{name}: restatement {ours:.2f} dB, PIL's own encode {pils:.2f} dB")
        assert ours >= pils - 0.5


def test_flat_frames_at_quality_100_decode_to_within_one_level():
    pytest.importorskip("PIL.Image")
    for rgb in [(90, 140, 200), (0, 0, 0), (255, 255, 255), (17, 250, 3), (128, 128, 128)]:
        f = mc.flat(24, 20, rgb)
        got = np.asarray(_decode(mr.encode(f, 100))).astype(int)
        assert np.abs(got - f).max() <= 1, (rgb, np.abs(got - f).max())


# ------------------------------------------------------------------ the AVI writer
def _wav_int16(path, rate, seconds, channels, seed):
    from scipy.io import wavfile
    pcm = np.random.default_rng(seed).integers(-32768, 32768, (int(rate * seconds), channels), dtype=np.int16)
    wavfile.write(str(path), rate, pcm if channels > 1 else pcm[:, 0])
    return pcm


@pytest.mark.parametrize("rate,channels,seconds", [(16000, 1, 0.25), (48000, 2, 0.25), (16000, 1, 0.05), (44100, 1, 0.11)])
def test_avi_round_trip(tmp_path, rate, channels, seconds):
    """frames from the restatement (odd and even lengths among them), an int16 WAV at a rate 30 does not divide (16000: 533.33 samples per frame), one it does
    (48000), a WAV shorter than the motion, and one with a tail beyond it"""
    jpegs = [f for name in ("noise_16x8_q50", "noise_16x8_q90", "noise_16x8_q100", "coef63_16x8_q50") for f in mc.reference(name)["files"]] * 2
    assert {len(j) % 2 for j in jpegs} == {0, 1}
    pcm = _wav_int16(tmp_path / "a.wav", rate, seconds, channels, 5)
    loaded, r = video.load_pcm16(tmp_path / "a.wav")
    assert r == rate and loaded.dtype == np.int16 and (loaded == pcm).all()
    path = tmp_path / "v.avi"
    with video.AviWriter(path, 16, 8, 30, (loaded, r)) as w:
        for j in jpegs:
            w.write_frame(j)
    mr.check_avi(path.read_bytes(), jpegs, 16, 8, 30, pcm, rate)
    with video.AviWriter(path, 16, 8, 30, None) as w:                                        # no waveform at hand: the video stream alone
        for j in jpegs[:3]:
            w.write_frame(j)
    mr.check_avi(path.read_bytes(), jpegs[:3], 16, 8, 30, None, 0)


def test_audio_of_other_formats_goes_through_the_loader(tmp_path):
    from scipy.io import wavfile
    x = np.array([0.0, 0.5, -0.5, 0.999999, -1.0, 1.0, 1e-5, -1e-5, 0.25 + 1 / 65536], np.float32)
    wavfile.write(str(tmp_path / "f.wav"), 22050, x)
    pcm, rate = video.load_pcm16(tmp_path / "f.wav")
    assert rate == 22050 and pcm.shape == (len(x), 1)
    assert pcm[:, 0].tolist() == np.clip(np.rint(x.astype(np.float64) * 32768), -32768, 32767).astype(int).tolist() and pcm[5, 0] == 32767 and pcm[4, 0] == -32768
    wavfile.write(str(tmp_path / "i.wav"), 8000, np.array([[0, -2 ** 31], [2 ** 30, 65536 * 3]], np.int32))
    pcm, rate = video.load_pcm16(tmp_path / "i.wav")
    assert rate == 8000 and pcm.tolist() == [[0, -32768], [16384, 3]]


def test_size_refusal(tmp_path, monkeypatch):
    j = mc.reference("noise_16x8_q90")["files"][0]
    w = video.AviWriter(tmp_path / "big.avi", 16, 8)
    w.write_frame(j)
    monkeypatch.setattr(video, "AVI_MAX_BYTES", w.f.tell() + 8 + len(j) + (len(j) & 1) + 8 + 32 - 1)      # one byte short of a second frame and its index
    with pytest.raises(ValueError, match="would pass"):
        w.write_frame(j)
    w.close()
    mr.check_avi((tmp_path / "big.avi").read_bytes(), [j], 16, 8, 30, None, 0)                               # what was in stays a valid file
    monkeypatch.setattr(video, "AVI_MAX_BYTES", 2 ** 31 - 1)
    assert video.AVI_MAX_BYTES == 2147483647
    with pytest.raises(ValueError):
        video.AviWriter(tmp_path / "x.avi", 16, 8, 29.97)
    with pytest.raises(ValueError):
        video.AviWriter(tmp_path / "x.avi", 16, 8, 30, (np.zeros((4, 1), np.float32), 16000))


def test_size_refusal_with_audio_leaves_a_valid_file(tmp_path, monkeypatch):
    """the frame fits, the audio tail behind it does not: close() still writes the index and the sizes, then raises the refusal"""
    j = mc.reference("noise_16x8_q90")["files"][0]
    pcm = np.random.default_rng(2).integers(-32768, 32768, (4000, 1), dtype=np.int16)       # 0.25 s at 16 kHz against ONE frame: 533 samples interleaved, 3467 in the tail
    for refused_in in ("write_frame", "close"):
        path = tmp_path / f"{refused_in}.avi"
        w = video.AviWriter(path, 16, 8, 30, (pcm, 16000))
        w.write_frame(j)
        if refused_in == "write_frame":      # (as inside Previewer.preview: the refusal, then `finally: avi.close()`)
            monkeypatch.setattr(video, "AVI_MAX_BYTES", w.f.tell() + 100)
            with pytest.raises(ValueError, match="would pass"):
                w.write_frame(j)
        else:
            monkeypatch.setattr(video, "AVI_MAX_BYTES", w.f.tell() + 8 + 3467 * 2 + 8 + 48 - 1)     # one byte short of the tail and its index
        with pytest.raises(ValueError, match="would pass"):
            w.close()
        assert w.f is None
        monkeypatch.setattr(video, "AVI_MAX_BYTES", 2 ** 31 - 1)
        mr.check_avi(path.read_bytes(), [j], 16, 8, 30, pcm[:533], 16000)                    # what was in: the frame and its own 533 samples
        w.close()                                                                            # closed is closed


# ------------------------------------------------------------------ dataset-driven edits: the take's ld_waveform, clip by clip
def test_dataset_jobs_carry_ld_waveform_per_clip():
    import torch
    from amuse_amd.trainer import emotion_control_jobs, preview_audio_of_job, style_transfer_jobs, style_Xemo_transfer_jobs
    g = torch.Generator().manual_seed(0)
    z = lambda n: torch.randn(n, 256, generator=g)

    def take(a, n, wave):
        e = {"ld_z": torch.zeros(n, 128), "ld_z_con": z(n), "ld_z_emo": z(n), "ld_z_sty": z(n), "ld_attr": (a, "male", "native", "x", "30"),
             "ld_wav": np.arange(n * 10000), "ld_motion": None}
        if wave is not None:
            e["ld_waveform"] = wave
        return e
    wave = torch.linspace(-1.0, 1.0, 2 * 160000 + 5000)[None]                                # (1, n): two clips and a rest
    takes = ["0_9_9", "0_65_65"]
    for has in (True, False):
        data = {"wayne": {t: take("wayne", 2, wave if has else None) for t in takes}}
        for t in takes:
            for o in takes:
                if o != t:
                    data["wayne"][t][f"ld_z_emo_{o}"] = data["wayne"][o]["ld_z_emo"]
        jobs = emotion_control_jobs(data, "first")
        assert len(jobs) == 4 and all(len(j["audio"]) == 20000 for j in jobs)                # ld_wav stays what the reference slices; it is not the preview's audio
        for j in jobs:
            got = preview_audio_of_job(j, j["bsz"])
            if not has:
                assert got == [None, None] and j["waveform"] is None                         # no ld_waveform in the dictionary: the video stream alone
                continue
            assert [(a[0], a[2]) for a in got] == [("ld_waveform", 0), ("ld_waveform", 1)] and all(a[1] is wave for a in got)      # by reference, nothing converted
            for tag, w, c in got:
                pcm, rate = video.clip_pcm16(w, c)
                assert rate == 16000 and pcm.shape == (160000, 1) and pcm.dtype == np.int16
                want = np.clip(np.rint(wave[0, c * 160000:(c + 1) * 160000].double().numpy() * 32768), -32768, 32767)
                assert (pcm[:, 0] == want).all()
    assert preview_audio_of_job(None, 2) == [None, None]
    pcm, _ = video.clip_pcm16(wave, 2)
    assert pcm.shape == (5000, 1) and video.clip_pcm16(wave, 3) is None                      # a waveform that ends early ends early; beyond it: nothing
    assert video.clip_pcm16(np.zeros(160000, np.float32), 0)[0].shape == (160000, 1)         # (n,) arrays too
    stereo = video.clip_pcm16(np.stack([np.full(200000, 0.5), np.full(200000, -0.25)]), 1)[0]
    assert stereo.shape == (40000, 2) and stereo[0].tolist() == [16384, -8192]
    # the transfer tasks carry their take's waveform the same way
    st = {a: {t: take(a, 2, wave) for t in ("0_73_73", "0_74_74")} for a in ("lu", "lawrence")}
    for t in ("0_73_73", "0_74_74"):
        for a, b in (("lu", "lawrence"), ("lawrence", "lu")):
            st[a][t][f"ld_z_sty_{b}"], st[a][t][f"ld_z_emo_{b}"] = st[b][t]["ld_z_emo"], st[b][t]["ld_z_sty"]
    assert all(j["waveform"] is wave for j in style_transfer_jobs(st, "[lu-lawrence]", "[angry]"))
    sx = {a: {t: take(a, 1, wave if a == "scott" else None) for t in ("0_65_65", "0_73_73")} for a in ("scott", "lu")}
    t1, t2 = "0_65_65", "0_73_73"
    for (xa, xt), (ya, yt) in ((("scott", t1), ("lu", t2)), (("lu", t1), ("scott", t2)), (("scott", t2), ("lu", t1)), (("lu", t2), ("scott", t1))):
        sx[xa][xt][f"ld_z_emo_{ya}_{yt}"], sx[xa][xt][f"ld_z_sty_{ya}_{yt}"] = sx[ya][yt]["ld_z_emo"], sx[ya][yt]["ld_z_sty"]
    sx["takes"] = f"{t1}*{t2}*{t1}*{t2}"
    xj = style_Xemo_transfer_jobs(sx, "[scott-lu]", "[happy-angry]")
    assert [j["waveform"] is wave for j in xj] == [j["actor"] == "scott" for j in xj] and any(j["waveform"] is None for j in xj)      # the content take's own, or none


# ------------------------------------------------------------------ the command lines
def test_cli_refusals(tmp_path):
    from amuse_amd import main as amain
    from amuse_amd import render
    for argv, msg in [(["--fn", "infer_gesture", "--preview-video"], "--preview-video belongs to --preview"),
                      (["--fn", "infer_gesture", "--preview", "--preview-quality", "80"], "--preview-quality belongs to --preview-video"),
                      (["--fn", "infer_gesture", "--preview", "--preview-video", "--preview-quality", "0"], "outside 1..100"),
                      (["--fn", "infer_gesture", "--preview", "--preview-video", "--preview-quality", "101"], "outside 1..100"),
                      (["--fn", "train_gesture", "--preview-video"], "--preview belongs to --fn infer_gesture / edit_gesture")]:
        with pytest.raises(SystemExit) as e:
            amain.main(argv)
        assert msg in str(e.value), (argv, e.value)
    for argv, msg in [(["a.npz", "--smplx-models", str(tmp_path), "--audio", "a.wav"], "belong to --video"),
                      (["a.npz", "--smplx-models", str(tmp_path), "--quality", "80"], "belong to --video"),
                      (["a.npz", "--smplx-models", str(tmp_path), "--video", "--quality", "0"], "outside 1..100"),
                      (["a.npz", "b.npz", "--smplx-models", str(tmp_path), "--video", "--audio", "a.wav"], "ONE motion"),
                      (["a.npz", "--smplx-models", str(tmp_path), "--video", "--audio", str(tmp_path / "missing.wav")], "does not exist")]:
        with pytest.raises(SystemExit) as e:
            render.main(argv)
        assert msg in str(e.value), (argv, e.value)
