"""Inputs of the preview video encoder's tests (tests/test_mjpeg_cpu.py, tests/test_gpu_mjpeg.py): seeded frames at the smallest shapes that still reach every
branch of the encoder, and - on the restatement alone (tests/mjpeg_ref.py) - the assertion that every case really exercises the branch it is there for, so a
case that stops doing so fails on the CPU.

Shapes, width x height: 16 x 8 (one interval, no RST), 24 x 20 (the last row repeated, three intervals), 21 x 19 (added: the last column AND the last row
repeated - 24 is a multiple of 8), 40 x 72 (nine intervals: RST0 .. RST7 all occur), 16 x 88 (added: eleven intervals, so the RST number really goes round to 0
again).  Qualities 50, 90, 100."""
import functools

import numpy as np

import mjpeg_ref as mr

# seeds of the noise cases: the first at which the restatement's output holds a stuffed FF 00 (small frames often hold no 0xFF byte at all)
NOISE_SEEDS = {"16x8_q50": 166, "24x20_q50": 174, "40x72_q50": 190, "16x8_q90": 212, "24x20_q90": 214, "21x19_q90": 212, "40x72_q90": 230, "16x88_q90": 206,
               "16x8_q100": 216, "24x20_q100": 224, "40x72_q100": 240}
SHAPES = {"16x8": (16, 8), "24x20": (24, 20), "21x19": (21, 19), "40x72": (40, 72), "16x88": (16, 88)}


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], -1).astype(np.uint8)


def flat(w, h, rgb=(90, 140, 200)):
    return np.broadcast_to(np.asarray(rgb, np.uint8), (h, w, 3)).copy()


def single_coefficient(w, h, natural_index, amplitude):
    """grey frames whose every 8 x 8 block is 128 + the inverse transform of ONE coefficient: after quantisation only that coefficient (and DC) survives"""
    D = mr.dct_matrix()
    F = np.zeros((8, 8))
    F[natural_index // 8, natural_index % 8] = amplitude
    blk = np.clip(np.rint(128 + D.T @ F @ D), 0, 255).astype(np.uint8)
    img = np.tile(blk, (-(-h // 8), -(-w // 8)))[:h, :w]
    return np.repeat(img[..., None], 3, -1)


def black_white(w, h):
    """8-pixel columns alternating black and white: at quality 100 the luma DC jumps by 2040, a difference of category 11"""
    x = np.arange(w) // 8 % 2
    return np.broadcast_to((x * 255).astype(np.uint8)[None, :, None], (h, w, 3)).copy()


@functools.lru_cache(maxsize=None)
def render_frame():
    """one frame of the renderer's synthetic model (tests/render_cases.py), rendered by the renderer's restatement: 64 x 48"""
    import render_cases as rc
    import render_ref as rr
    b = rc.body_case(frames=1)
    rgb = rr.render(b["v64"][0], b["faces"], b["cam"], b["width"], b["height"], 2)[0]
    return np.ascontiguousarray(rgb.astype(np.uint8))


def _cases():
    c = {}
    for q in (50, 90, 100):
        for s, (w, h) in SHAPES.items():
            if s in ("21x19", "16x88") and q != 90:
                continue
            c[f"noise_{s}_q{q}"] = (lambda w=w, h=h, seed=NOISE_SEEDS[f"{s}_q{q}"]: noise(w, h, seed)[None], q, {"stuffed", "rst" if h > 8 else "no_rst"})
    c["ramp_40x72_q50"] = (lambda: ramp(40, 72)[None], 50, {"rst_wraps"})
    c["ramp_21x19_q90"] = (lambda: ramp(21, 19)[None], 90, set())
    c["flat_24x20_q100"] = (lambda: flat(24, 20)[None], 100, {"flat"})
    c["highfreq_24x20_q50"] = (lambda: single_coefficient(24, 20, int(mr.ZIGZAG[40]), 300.0)[None], 50, {"zrl"})
    c["coef63_16x8_q50"] = (lambda: single_coefficient(16, 8, 63, 400.0)[None], 50, {"no_eob", "zrl"})
    c["blackwhite_24x20_q100"] = (lambda: black_white(24, 20)[None], 100, {"dc11"})
    c["render_64x48_q90"] = (lambda: render_frame()[None], 90, set())
    c["batch3_24x20_q90"] = (lambda: np.stack([noise(24, 20, 7), ramp(24, 20), flat(24, 20)]), 90, {"batch"})
    return c


CASES = _cases()
NAMES = list(CASES)


def quality(name):
    return CASES[name][1]


@functools.lru_cache(maxsize=None)
def frames(name):
    """uint8 [M, H, W, 3]; computed once, never written to"""
    f = np.ascontiguousarray(CASES[name][0]())
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's answers for a case, computed once and shared: quotients (float64 F / t), coef (int16), files (bytes per frame), events (per frame)"""
    fr, q = frames(name), quality(name)
    quot = np.stack([mr.quotients(f, q) for f in fr])
    coef = mr.quantise(quot)
    events = [dict() for _ in fr]
    H, W = fr.shape[1:3]
    files = [mr.encode_coefficients(coef[m], W, H, q, events[m]) for m in range(len(fr))]
    for a in (quot, coef):
        a.setflags(write=False)
    return {"quotients": quot, "coef": coef, "files": files, "events": events}


def check_exercises_its_branch(name):
    """asserts, on the restatement alone, that the case reaches what it is there for"""
    want, ref, fr = CASES[name][2], reference(name), frames(name)
    ev, data = ref["events"][0], ref["files"][0]
    scan = data[mr.HEADER_BYTES:-2]
    rst = [scan[i + 1] & 7 for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    mcus_y = -(-fr.shape[1] // 8)
    assert len(rst) == mcus_y - 1 and rst == [k % 8 for k in range(mcus_y - 1)], (name, rst)
    if "stuffed" in want:
        assert b"\xFF\x00" in scan, name
    if "no_rst" in want:
        assert mcus_y == 1 and not rst
    if "rst" in want:
        assert len(rst) >= 2
    if "rst_wraps" in want:
        assert len(rst) == 8 and rst[-1] == 7 and mcus_y == 9          # RST0 .. RST7
    if name.startswith("noise_16x88"):
        assert rst == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1]
    if "flat" in want:
        blocks = 3 * mcus_y * -(-fr.shape[2] // 8)
        assert ev.get("eob_only") == blocks and ev.get("dc_zero", 0) >= blocks - 3 * mcus_y and (ref["coef"][0][..., 1:] == 0).all()
    if "zrl" in want:
        assert ev.get("zrl", 0) >= 1, (name, ev)
    if "no_eob" in want:
        assert ev.get("no_eob", 0) >= 1 and (ref["coef"][0][..., 63] != 0).any(), (name, ev)
    if "dc11" in want:
        assert ev.get("max_dc_category") == 11, (name, ev)
    if "batch" in want:
        assert len(fr) == 3 and len({bytes(f) for f in ref["files"]}) == 3
    if name.startswith("render"):
        assert len(np.unique(fr[0].reshape(-1, 3), axis=0)) > 10          # a picture, not a flat field
