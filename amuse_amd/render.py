"""Preview rendering: the posed SMPL-X mesh rasterised to PNG frames in HIP (include/amuse_hip.h amuse_render, csrc/k_render.hip).

AN EXTENSION, off by default.  The reference hands its NPZ to Blender (1024 x 1024, 75 mm lens, front camera) and the frames to ffmpeg; neither is rebuilt here.
This is a PREVIEW: the mesh flat-shaded from one fixed front camera, so that a result can be looked at without Blender and the SMPL-X add-on.  It matches no
other renderer's image and is checked against its own restatement only (tests/render_ref.py).

    python -m amuse_amd.render FILE_motion_smplx.npz --smplx-models DIR [--size 512] [--stride 10] [--frames] [--video [--audio FILE.wav] [--quality 90]]

writes FILE_preview.png (a contact sheet of every stride-th frame) beside the NPZ, with --frames also FILE_preview/frame_%04d.png; `main.py --preview` does the
same for every NPZ a run writes.  With --video [--audio FILE.wav] [--quality 90] EVERY frame also goes, still on the device, through the HIP JPEG encoder of
amuse_amd/video.py into FILE_preview.avi (Motion-JPEG, with the WAV's own samples as 16-bit PCM when one is given).  The model files must carry their triangles (key 'f', as the published SMPL-X files do).  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from contextlib import closing
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _lib, body, motion_file

LENS_MM, SENSOR_MM = 75.0, 36.0     # the reference's Blender camera: a 75 mm lens on the default 36 mm sensor
FLESH_PAD = 0.15                    # metres added around the joints' bounding box: the joints lie inside the body
SHEET_COLS = 6


def plan(width: int, height: int, ss: int, V: int, T: int, frames: int) -> dict:
    """amuse_render_plan: the library's own statement of the tile grid, the frames per chunk and the workspace; no GPU needed."""
    tx, ty, ch, ws = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    _lib.check(_lib.load().amuse_render_plan(int(width), int(height), int(ss), int(V), int(T), int(frames), C.byref(tx), C.byref(ty), C.byref(ch), C.byref(ws)))
    return {"tiles_x": tx.value, "tiles_y": ty.value, "chunk_frames": ch.value, "workspace_bytes": ws.value}


class Camera:
    """x_cam = R x + t, looking down +z_cam with y_cam up; u = fx x / z + cx, v = cy - fy y / z (pixel (i, j) has its centre at u = i + 0.5, v = j + 0.5)."""

    def __init__(self, R, t, fx, fy, cx, cy, near, far):
        self.R = np.asarray(R, np.float64).reshape(3, 3)
        self.t = np.asarray(t, np.float64).reshape(3)
        self.fx, self.fy, self.cx, self.cy, self.near, self.far = (float(x) for x in (fx, fy, cx, cy, near, far))

    @classmethod
    def front(cls, points, width: int, height: int, margin: float = 0.1, distance: Optional[float] = None) -> "Camera":
        """A fixed front camera for a whole clip: on the +z side of the body (SMPL-X faces +z, y up), looking along -z, aimed at the centre of the bounding box of
        `points` ([..., 3]: the clip's posed joints over ALL frames), with the reference's 75 mm lens.  The box, grown by `margin` of its size and by 0.15 m for the
        flesh around the joints, fits the image at the depth of its front face; `distance` (box centre to camera) overrides that.  World +x is image right."""
        p = np.asarray(points, np.float64).reshape(-1, 3)
        lo, hi = p.min(0), p.max(0)
        c, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * (1.0 + margin) + FLESH_PAD
        f = LENS_MM / SENSOR_MM * max(width, height)
        if distance is None:
            distance = max(half[0] * f / (0.5 * width), half[1] * f / (0.5 * height)) + half[2]
        reach = float(np.linalg.norm(half)) + 0.5
        R = np.diag([1.0, 1.0, -1.0])
        eye = c + np.array([0.0, 0.0, distance])
        return cls(R, -R @ eye, f, f, 0.5 * width, 0.5 * height, max(0.05, distance - reach), distance + reach)

    def to_c(self) -> "_lib.CameraC":
        c = _lib.CameraC()
        c.R[:] = [float(x) for x in self.R.reshape(-1)]
        c.t[:] = [float(x) for x in self.t]
        c.fx, c.fy, c.cx, c.cy, c.near_z, c.far_z = self.fx, self.fy, self.cx, self.cy, self.near, self.far
        return c


class Shading:
    """c = ambient + (1 - ambient) |n . light|; the defaults are the library's (a headlight)."""

    def __init__(self, light=(0.0, 0.0, -1.0), ambient: float = 0.25, body_rgb=(200, 200, 208), bg_rgb=(32, 32, 36)):
        self.light, self.ambient, self.body_rgb, self.bg_rgb = tuple(float(x) for x in light), float(ambient), tuple(int(x) for x in body_rgb), tuple(int(x) for x in bg_rgb)

    def to_c(self) -> "_lib.ShadingC":
        s = _lib.ShadingC()
        s.light[:] = self.light
        s.ambient = self.ambient
        s.body_rgb[:] = self.body_rgb
        s.bg_rgb[:] = self.bg_rgb
        return s


class Renderer:
    """One mesh topology at one image size on one GPU.  Calls are stream-ordered on torch's current stream; the first call of a size allocates the workspace."""

    def __init__(self, device, faces, V: int, width: int, height: int, ss: int = 2):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AmuseHipError("amuse_amd.render has no CPU fallback: the renderer is a HIP kernel (tests/render_ref.py is a test's restatement, not a renderer)")
        fc = np.ascontiguousarray(np.asarray(faces).astype(np.int64).astype(np.int32).reshape(-1, 3))
        self.T, self.V, self.width, self.height, self.ss = int(fc.shape[0]), int(V), int(width), int(height), int(ss)
        self.ctx = self.lib.amuse_renderer_create(self.device.index or 0, fc.ctypes.data_as(C.POINTER(C.c_int)), self.T, self.V, self.width, self.height, self.ss)
        if not self.ctx:
            raise _lib.AmuseHipError(f"amuse_renderer_create: {self.lib.amuse_last_error().decode()}")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.amuse_renderer_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def render(self, vertices, camera: Camera, shading: Optional[Shading] = None, keys: bool = False, screen: bool = False):
        """vertices: device float32 [M, V, 3] -> uint8 [M, H, W, 3]; with keys / screen a tuple (rgb[, keys int64 [M, H ss, W ss]: the winning keys' 64 bits, -1 =
        empty][, screen int32 [M, V, 3]])."""
        assert vertices.is_cuda and vertices.dtype == torch.float32 and vertices.is_contiguous() and vertices.dim() == 3 and tuple(vertices.shape[1:]) == (self.V, 3), \
            f"vertices: device float32 [M, {self.V}, 3], contiguous"
        M = int(vertices.shape[0])
        rgb = torch.empty(M, self.height, self.width, 3, dtype=torch.uint8, device=self.device)
        ko = torch.empty(M, self.height * self.ss, self.width * self.ss, dtype=torch.int64, device=self.device) if keys else None
        so = torch.empty(M, self.V, 3, dtype=torch.int32, device=self.device) if screen else None
        cam = camera.to_c()
        sh = shading.to_c() if shading is not None else None
        _lib.check(self.lib.amuse_render(self.ctx, vertices.data_ptr(), M, C.byref(cam), C.byref(sh) if sh is not None else None, rgb.data_ptr(),
                                         ko.data_ptr() if keys else None, so.data_ptr() if screen else None, self._stream()))
        out = (rgb,) + ((ko,) if keys else ()) + ((so,) if screen else ())
        return out[0] if len(out) == 1 else out

    def raster(self, screen):
        """tests: the raster stage alone on caller-made records, device int32 [M, V, 3] -> keys int64 [M, H ss, W ss]"""
        assert screen.is_cuda and screen.dtype == torch.int32 and screen.is_contiguous() and tuple(screen.shape[1:]) == (self.V, 3)
        M = int(screen.shape[0])
        ko = torch.empty(M, self.height * self.ss, self.width * self.ss, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.amuse_debug_render_raster(self.ctx, screen.data_ptr(), M, ko.data_ptr(), self._stream()))
        return ko


# ------------------------------------------------------------------ PNG, on the standard library alone
def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_bytes(array) -> bytes:
    """uint8 [H, W, 3] (RGB) or [H, W] (grey) -> the bytes of an 8-bit, non-interlaced PNG (filter 0 on every row, zlib level 6: the same bytes on every machine
    with the same zlib)."""
    a = np.ascontiguousarray(np.asarray(array))
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: uint8 [H, W, 3] or [H, W], got {a.dtype} {tuple(a.shape)}")
    h, w = a.shape[:2]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, -1)], axis=1)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b"")


def write_png(path, array) -> None:
    Path(path).write_bytes(png_bytes(array))


def contact_sheet(frames, cols: int = SHEET_COLS):
    """uint8 [N, H, W, 3] -> [ceil(N / cols) H, cols W, 3], row-major; cells past the last frame take frame 0's top-left pixel (the background)."""
    f = np.asarray(frames)
    assert f.ndim == 4 and f.shape[0] >= 1 and cols >= 1, f.shape
    n, h, w, ch = f.shape
    cols = min(cols, n)
    rows = -(-n // cols)
    sheet = np.empty((rows * cols, h, w, ch), f.dtype)
    sheet[:n] = f
    sheet[n:] = f[0, 0, 0]
    return np.ascontiguousarray(sheet.reshape(rows, cols, h, w, ch).transpose(0, 2, 1, 3, 4).reshape(rows * h, cols * w, ch))


# ------------------------------------------------------------------ NPZ -> pictures
def load_preview_models(directory) -> dict:
    """{"male" | "female" | "neutral": BodyModel with faces} from a directory of the user's SMPL-X files; SystemExit names what is missing."""
    return body.require_models(directory, "preview: ", "(--smplx-models DIR names another directory): the preview poses the licensed SMPL-X body models", faces=True)


def preview_paths(npz_path, out_dir=None):
    """(sheet, frames directory) of an NPZ: <name>_motion_smplx.npz -> <name>_preview.png, <name>_preview/"""
    return motion_file.sibling(npz_path, "_preview.png", out_dir), motion_file.sibling(npz_path, "_preview", out_dir)


class Previewer:
    """The body engines and renderers of a run, built once per gender: preview(npz) poses the file's poses / trans / betas / gender and writes its pictures."""

    def __init__(self, models: dict, device="cuda:0", size: int = 512, stride: int = 10, frames: bool = False, ss: int = 2, batch: int = 64, video: bool = False,
                 quality: int = 90):
        if size < 1 or stride < 1:
            raise SystemExit(f"preview: --preview-size {size} and --preview-stride {stride} must be >= 1")
        if video and not 1 <= quality <= 100:
            raise SystemExit(f"preview: --quality {quality} outside 1..100")
        self.models, self.device, self.size, self.stride, self.frames, self.ss, self.batch = models, torch.device(device), int(size), int(stride), bool(frames), ss, batch
        self.video, self.quality, self._enc = bool(video), int(quality), None
        self._poser, self._ren = body.Poser(models, self.device), {}

    def close(self):
        self._poser.close()
        for r in self._ren.values():
            r.close()
        self._ren = {}
        if self._enc is not None:
            self._enc.close()
            self._enc = None

    def _video_writer(self, path, wav):
        """video=True: the AVI of one NPZ; wav = a WAV file, (int16 [samples, channels], rate), or None for a video stream alone"""
        from . import video
        if self._enc is None:
            self._enc = video.JpegEncoder(self.device, self.size, self.size, self.quality)
        audio = video.load_pcm16(wav) if isinstance(wav, (str, Path)) else wav
        return video.AviWriter(path, self.size, self.size, 30, audio)

    def preview(self, npz_path, out_dir=None, wav=None):
        """-> the paths written (the sheet first; with video=True the AVI last)"""
        m = motion_file.read(npz_path)
        if m.gender not in self.models:
            m = m._replace(gender="neutral")
        model = self.models[m.gender]
        if model.faces is None:
            raise SystemExit(f"preview: the {m.gender} body model lacks the key 'f' (the mesh's triangles)")
        eng, rot, tr = self._poser.pose(m)
        if m.gender not in self._ren:
            self._ren[m.gender] = Renderer(self.device, model.faces, model.V, self.size, self.size, self.ss)
        ren, F = self._ren[m.gender], int(rot.shape[1])
        cam = Camera.front(eng.joints(rot, tr).cpu().numpy(), self.size, self.size)      # one camera for the clip: framed on every frame's joints
        sheet_path, frames_dir = preview_paths(npz_path, out_dir)
        sheet_path.parent.mkdir(parents=True, exist_ok=True)
        # the video takes EVERY frame; the host keeps what the pictures need: every frame with frames=True, every stride-th otherwise
        picked = list(range(F)) if (self.frames or self.video) else list(range(0, F, self.stride))
        kept = picked if self.frames else list(range(0, F, self.stride))
        out = np.empty((len(kept), self.size, self.size, 3), np.uint8)
        idx = torch.tensor(picked, device=self.device)
        avi = self._video_writer(sheet_path.with_suffix(".avi"), wav) if self.video else None
        try:
            for i0 in range(0, len(picked), self.batch):
                sel = idx[i0:i0 + self.batch]
                v = eng.vertices(rot[:, sel].contiguous(), tr[:, sel].contiguous())[0]
                rgb = ren.render(v, cam)
                if avi is not None:
                    for jpeg in self._enc.encode(rgb):      # the frames never leave the device as raw RGB for the video
                        avi.write_frame(jpeg)
                if len(kept) == len(picked):
                    out[i0:i0 + self.batch] = rgb.cpu().numpy()
                else:
                    local = [i for i in range(int(sel.numel())) if picked[i0 + i] % self.stride == 0]
                    if local:
                        out[[picked[i0 + i] // self.stride for i in local]] = rgb[torch.tensor(local, device=self.device)].cpu().numpy()
        finally:
            if avi is not None:
                avi.close()
        sheet = out[::self.stride] if self.frames else out
        write_png(sheet_path, contact_sheet(sheet, SHEET_COLS))
        written = [sheet_path]
        if self.frames:
            frames_dir.mkdir(parents=True, exist_ok=True)
            for f in range(F):
                write_png(frames_dir / f"frame_{f:04d}.png", out[f])
                written.append(frames_dir / f"frame_{f:04d}.png")
        if avi is not None:
            written.append(avi.path)
        return written


def preview_npz(npz_path, models, out_dir=None, size: int = 512, stride: int = 10, frames: bool = False, device="cuda:0", video: bool = False, quality: int = 90,
                wav=None):
    """One NPZ (this project's or the reference's own): models = {"male" | "female" | "neutral": BodyModel} or a directory holding the SMPL-X files."""
    if not isinstance(models, dict):
        models = load_preview_models(models)
    with closing(Previewer(models, device, size, stride, frames, video=video, quality=quality)) as p:
        return p.preview(npz_path, out_dir, wav)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="preview of a *_motion_smplx.npz: a contact sheet (and frames) of the posed SMPL-X mesh, rendered in HIP")
    ap.add_argument("npz", nargs="+")
    ap.add_argument("--smplx-models", required=True, help="directory holding SMPLX_MALE.npz, SMPLX_FEMALE.npz, SMPLX_NEUTRAL.npz (with their 'f')")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--stride", type=int, default=10, help="every stride-th frame goes on the sheet")
    ap.add_argument("--frames", action="store_true", help="also write <name>_preview/frame_%%04d.png for every frame")
    ap.add_argument("--out-dir", default=None, help="default: beside the NPZ")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--video", action="store_true", help="also write <name>_preview.avi: every frame as Motion-JPEG, encoded in HIP kernels (amuse_amd/video.py)")
    ap.add_argument("--audio", default=None, help="--video: the WAV whose own samples the AVI carries as 16-bit PCM (one NPZ only)")
    ap.add_argument("--quality", type=int, default=None, help="--video: JPEG quality 1..100 (default 90)")
    args = ap.parse_args(argv)
    if (args.audio is not None or args.quality is not None) and not args.video:
        raise SystemExit("preview: --audio and --quality belong to --video")
    quality = 90 if args.quality is None else args.quality
    if not 1 <= quality <= 100:
        raise SystemExit(f"preview: --quality {quality} outside 1..100")
    if args.audio is not None and len(args.npz) != 1:
        raise SystemExit(f"preview: --audio names the WAV of ONE motion; {len(args.npz)} NPZ files were given")
    if args.audio is not None and not Path(args.audio).is_file():
        raise SystemExit(f"preview: {args.audio} does not exist")
    models = load_preview_models(args.smplx_models)
    for n in args.npz:
        if not Path(n).is_file():
            raise SystemExit(f"preview: {n} does not exist")
    with closing(Previewer(models, args.device, args.size, args.stride, args.frames, video=args.video, quality=quality)) as p:
        written = [f for n in args.npz for f in p.preview(n, args.out_dir, args.audio)]
    n_avi = sum(1 for w in written if Path(w).suffix == ".avi")
    print(f"preview: wrote {len(written) - n_avi} PNG files" + (f" and {n_avi} AVI files" if n_avi else "") + f"; first {written[0]}")
    return written


if __name__ == "__main__":
    main()
