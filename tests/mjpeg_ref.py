"""A float64 / integer restatement of the preview video encoder (include/amuse_hip.h, "preview video"; csrc/amuse_mjpeg_host.hpp, csrc/k_mjpeg.hip), for tests:
the tables of a quality, colour + DCT + quantisation, the entropy coder (bit exact), the file header, and a small RIFF walker for AVI files.  Nothing here is
used by the package.  The constants are facts of ITU-T T.81 (Annex K.1 - K.3); tests/test_mjpeg_cpu.py holds them to PIL's wherever PIL imports."""
import struct

import numpy as np

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8 if (i // 8 + i % 8) % 2 else i % 8)))      # anti-diagonals, alternating direction
    return np.array(order)


ZIGZAG = _zigzag()                      # zigzag position k -> natural index 8 v + u
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
AC_LUMA_VALS = [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
                0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
                0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
                0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
                0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
                0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
                0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]
AC_CHROMA_VALS = [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
                  0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
                  0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
                  0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
                  0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
                  0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
                  0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
HUFFMAN = {0x00: (DC_LUMA_BITS, DC_VALS), 0x10: (AC_LUMA_BITS, AC_LUMA_VALS), 0x01: (DC_CHROMA_BITS, DC_VALS), 0x11: (AC_CHROMA_BITS, AC_CHROMA_VALS)}
HEADER_BYTES = 629
BLOCK_BITS = 1660


def tables(quality):
    """-> (luma, chroma) int [64] in natural order: libjpeg's rule on the Annex K base tables"""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((b * s + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA))


def plan(width, height, frames):
    mx, my = -(-width // 8), -(-height // 8)
    al = lambda n: -(-n // 256) * 256
    ws = al(frames * mx * my * 384) + 2 * al(frames * my * 4) + al(frames * 4)
    worst = HEADER_BYTES + my * 2 * -(-(mx * 3 * BLOCK_BITS) // 8) + 2 * (my - 1) + 2
    return {"mcus_x": mx, "mcus_y": my, "header_bytes": HEADER_BYTES, "workspace_bytes": ws, "worst_case_bytes_per_frame": worst}


def dct_matrix(dtype=np.float64):
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    d = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    d[0] *= 1 / np.sqrt(2)
    return d.astype(dtype)


def quotients(rgb, quality, dtype=np.float64):
    """uint8 [H, W, 3] -> F / t before rounding, [mcus_y, mcus_x, 3, 64] in zigzag order, in `dtype` (float64: the restatement; float32: what fp32 can reach)"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    H, W = rgb.shape[:2]
    my, mx = -(-H // 8), -(-W // 8)
    p = np.pad(rgb, ((0, my * 8 - H), (0, mx * 8 - W), (0, 0)), mode="edge").astype(dtype)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    c = lambda v: dtype(v)
    ycc = np.stack([c(0.299) * R + c(0.587) * G + c(0.114) * B - c(128), c(-0.168735892) * R - c(0.331264108) * G + c(0.5) * B,
                    c(0.5) * R - c(0.418687589) * G - c(0.081312411) * B])                                  # [3, Hp, Wp]
    blocks = ycc.reshape(3, my, 8, mx, 8).transpose(1, 3, 0, 2, 4)                                         # [my, mx, 3, y, x]
    D = dct_matrix(dtype)
    F = np.einsum("vy,abcyx,ux->abcvu", D, blocks, D).reshape(my, mx, 3, 64)                              # natural index 8 v + u
    tl, tc = tables(quality)
    t = np.stack([tl, tc, tc]).astype(dtype)                                                               # [3, 64] natural
    return (F / t[None, None])[..., ZIGZAG].astype(dtype)


def quantise(q):
    """round half away from zero; DC clamped to [-1024, 1023], AC to [-1023, 1023] -> int16"""
    r = np.trunc(q + np.copysign(0.5, q))
    r = np.clip(r, -1023, 1023)
    r[..., 0] = np.clip(np.trunc(q[..., 0] + np.copysign(0.5, q[..., 0])), -1024, 1023)
    return r.astype(np.int16)


def coefficients(rgb, quality):
    """uint8 [H, W, 3] -> int16 [mcus_y, mcus_x, 3, 64], zigzag order"""
    return quantise(quotients(rgb, quality))


def near_half(q, window):
    """True where F / t lies within `window` of a half-integer: there fp32 and float64 may round to different integers"""
    return np.abs(np.abs(q - np.floor(q)) - 0.5) <= window


def huffman_codes(bits, vals):
    """Annex C: symbol -> (code, length)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


CODES = {k: huffman_codes(*v) for k, v in HUFFMAN.items()}


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _category(v):
    return int(abs(int(v))).bit_length()


def encode_interval(coef_row, events=None):
    """int [mcus_x, 3, 64] (zigzag) -> the bytes of one restart interval (no RST marker).  `events`, a dict, counts what occurred."""
    w, pred = _Bits(), [0, 0, 0]
    ev = events if events is not None else {}
    for mcu in np.asarray(coef_row).astype(np.int64):
        for c in range(3):
            blk = mcu[c]
            dc, ac = CODES[0x00 if c == 0 else 0x01], CODES[0x10 if c == 0 else 0x11]
            d = int(blk[0]) - pred[c]
            pred[c] = int(blk[0])
            cat = _category(d)
            ev["max_dc_category"] = max(ev.get("max_dc_category", 0), cat)
            ev["dc_zero"] = ev.get("dc_zero", 0) + (d == 0)
            code, length = dc[cat]
            w.put((code << cat) | ((d - (d < 0)) & ((1 << cat) - 1)), length + cat)
            run = 0
            for k in range(1, 64):
                v = int(blk[k])
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    w.put(*ac[0xF0])
                    ev["zrl"] = ev.get("zrl", 0) + 1
                    run -= 16
                cat = _category(v)
                code, length = ac[(run << 4) | cat]
                w.put((code << cat) | ((v - (v < 0)) & ((1 << cat) - 1)), length + cat)
                run = 0
            if run:
                w.put(*ac[0x00])
                ev["eob"] = ev.get("eob", 0) + 1
                ev["eob_only"] = ev.get("eob_only", 0) + (run == 63)
            else:
                ev["no_eob"] = ev.get("no_eob", 0) + 1
    w.flush()
    return bytes(w.out)


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def header(width, height, quality):
    """SOI .. SOS"""
    tl, tc = tables(quality)
    h = b"\xFF\xD8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, t in enumerate((tl, tc)):
        h += _segment(0xDB, bytes([i]) + bytes(int(x) for x in t[ZIGZAG]))
    h += _segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for key in (0x00, 0x10, 0x01, 0x11):
        bits, vals = HUFFMAN[key]
        h += _segment(0xC4, bytes([key]) + bytes(bits) + bytes(vals))
    h += _segment(0xDD, struct.pack(">H", -(-width // 8)))
    h += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(h) == HEADER_BYTES
    return h


def entropy(coef, events=None):
    """int [mcus_y, mcus_x, 3, 64] -> the scan's bytes: the intervals with RSTm between them"""
    out = b""
    for k, row in enumerate(coef):
        if k:
            out += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        out += encode_interval(row, events)
    return out


def encode_coefficients(coef, width, height, quality, events=None):
    return header(width, height, quality) + entropy(coef, events) + b"\xFF\xD9"


def encode(rgb, quality, events=None):
    """uint8 [H, W, 3] -> a complete JPEG file"""
    H, W = np.asarray(rgb).shape[:2]
    return encode_coefficients(coefficients(rgb, quality), W, H, quality, events)


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return float("inf") if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


# ------------------------------------------------------------------ AVI: a RIFF walker
def riff_chunks(data, start, end):
    """[(fourcc, payload offset, size, list type or None)] of the chunks in data[start:end]; sizes are checked against `end` and odd sizes take a pad byte"""
    out, p = [], start
    while p < end:
        assert p + 8 <= end, f"chunk header at {p} crosses {end}"
        cc, size = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
        assert p + 8 + size <= end, f"chunk {cc} at {p}: {size} bytes cross {end}"
        out.append((cc, p + 8, size, data[p + 8:p + 12] if cc in (b"RIFF", b"LIST") else None))
        p += 8 + size + (size & 1)
    assert p == end or p == end + 1, (p, end)
    return out


def walk_avi(data):
    """-> dict(avih, streams [(strh bytes, strf bytes)], movi [(fourcc, payload offset, size)], idx1 [(fourcc, flags, offset, size)], movi_start = the offset of
    the 'movi' fourcc, order = the top-level chunk names)"""
    top = riff_chunks(data, 0, len(data))
    assert len(top) == 1 and top[0][0] == b"RIFF" and top[0][3] == b"AVI " and top[0][2] == len(data) - 8, top
    res = {"streams": [], "movi": [], "idx1": [], "order": []}
    for cc, off, size, lt in riff_chunks(data, 12, len(data)):
        res["order"].append(lt if cc == b"LIST" else cc)
        if cc == b"LIST" and lt == b"hdrl":
            for c2, o2, s2, l2 in riff_chunks(data, off + 4, off + size):
                if c2 == b"avih":
                    res["avih"] = data[o2:o2 + s2]
                elif c2 == b"LIST" and l2 == b"strl":
                    sub = {c3: data[o3:o3 + s3] for c3, o3, s3, _ in riff_chunks(data, o2 + 4, o2 + s2)}
                    res["streams"].append((sub[b"strh"], sub[b"strf"]))
        elif cc == b"LIST" and lt == b"movi":
            res["movi_start"] = off
            res["movi"] = [(c2, o2, s2) for c2, o2, s2, _ in riff_chunks(data, off + 4, off + size)]
        elif cc == b"idx1":
            assert size % 16 == 0
            res["idx1"] = [struct.unpack("<4sIII", data[off + 16 * i:off + 16 * i + 16]) for i in range(size // 16)]
    return res


def check_avi(data, jpegs, width, height, fps, pcm, rate):
    """the walker's view of a file the writer made: chunk order, padding, index, patched sizes, rates, payloads; -> the walk"""
    a = walk_avi(data)
    n = len(jpegs)
    assert a["order"] == [b"hdrl", b"movi", b"idx1"]
    avih = struct.unpack("<14I", a["avih"])
    assert avih[0] == 1000000 // fps and avih[4] == n and avih[6] == (2 if pcm is not None else 1) and avih[8:10] == (width, height) and avih[3] & 0x10
    assert len(a["streams"]) == avih[6]
    vh = struct.unpack("<4s4sIHHIIIIIIII4h", a["streams"][0][0])
    assert vh[:2] == (b"vids", b"MJPG") and vh[6:8] == (1, fps) and vh[9] == n
    bi = struct.unpack("<IiiHH4sIiiII", a["streams"][0][1])
    assert bi[:6] == (40, width, height, 1, 24, b"MJPG")
    video_chunks = [(o, s) for cc, o, s in a["movi"] if cc == b"00dc"]
    assert [data[o:o + s] for o, s in video_chunks] == list(jpegs)
    assert all(o % 2 == 0 for _, o, _ in a["movi"])                                          # every chunk starts on an even offset: odd payloads were padded
    assert avih[7] == max(s for _, _, s in a["movi"])
    if pcm is not None:
        ch = pcm.shape[1]
        ah = struct.unpack("<4s4sIHHIIIIIIII4h", a["streams"][1][0])
        assert ah[0] == b"auds" and ah[6:8] == (2 * ch, rate * 2 * ch) and ah[9] == pcm.shape[0] and ah[12] == 2 * ch
        assert struct.unpack("<HHIIHHH", a["streams"][1][1]) == (1, ch, rate, rate * 2 * ch, 2 * ch, 16, 0)
        audio_chunks = [(o, s) for cc, o, s in a["movi"] if cc == b"01wb"]
        assert b"".join(data[o:o + s] for o, s in audio_chunks) == pcm.astype("<i2").tobytes()   # bit for bit
        # interleaved per frame: chunk k carries [floor(k rate / fps), floor((k + 1) rate / fps)); the rest in one final chunk
        tags = [cc for cc, _, _ in a["movi"]]
        covered = min(pcm.shape[0], n * rate // fps)
        k_full = min(n, next((k for k in range(n) if (k + 1) * rate // fps > pcm.shape[0]), n))
        assert tags[:2 * k_full] == [b"00dc", b"01wb"] * k_full
        for k in range(k_full):
            assert audio_chunks[k][1] == ((k + 1) * rate // fps - k * rate // fps) * 2 * ch
        if pcm.shape[0] > covered:
            assert tags[-1] == b"01wb" and audio_chunks[-1][1] == (pcm.shape[0] - covered) * 2 * ch
    else:
        assert all(cc == b"00dc" for cc, _, _ in a["movi"])
    assert len(a["idx1"]) == len(a["movi"])
    for (cc, flags, off, size), (mcc, mo, ms) in zip(a["idx1"], a["movi"]):                  # idx1 offsets count from the 'movi' fourcc and land on their chunks
        assert cc == mcc and size == ms and flags == 0x10 and a["movi_start"] + off + 8 == mo
        assert data[a["movi_start"] + off:a["movi_start"] + off + 4] == cc
    return a
