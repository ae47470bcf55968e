"""CPU: the tail of AST_EVP behind the three encoders (include/amuse_hip.h "Audio model metrics") without a GPU - the parameter inventory against stock
torch modules, the C ABI (declared, exported, every refusal), the weight-stream packer of the last Linear against its documented index formula, the
checkpoint round trip, PretrainedLPDM_v1.collect_audio_metrics on an injected engine, and the host code (set_tail, reconstruct, encode_labels, destroy) as a
stand-alone program on the stubbed runtime under ASan / UBSan (tests/host_tail; nothing is loaded into python under a sanitizer)."""
import ctypes as C
import os
import pickle
import re
import subprocess
from collections import OrderedDict
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn as nn

REPO = Path(__file__).resolve().parents[1]
N_TAIL = 158950988


# ------------------------------------------------------------------------------------------------ parameters
class _Fusion(nn.Module):      # models/audio/AST_EVP.py FusionBlock, restated
    def __init__(self, d, out, n=2):
        super().__init__()
        self.layers = nn.ModuleList([nn.TransformerEncoderLayer(d_model=d, nhead=4) for _ in range(n)])
        self.norm = nn.LayerNorm(d)
        self.fc = nn.Linear(d, out)


class _Decoder(nn.Module):     # DecoderBlock
    def __init__(self, d, out, n=4):
        super().__init__()
        self.layers = nn.ModuleList([nn.TransformerEncoderLayer(d_model=d, nhead=4) for _ in range(n)])
        self.norm = nn.LayerNorm(d)
        self.projection = nn.Sequential(nn.Linear(d, d * 2), nn.ReLU(), nn.Linear(d * 2, out))


class _Heads(nn.Module):       # the classifier heads of ASTModel (audio_main_new.py:79-81)
    def __init__(self, L):
        super().__init__()
        self.mlp_head = nn.Sequential(nn.LayerNorm(256), nn.Linear(256, L))
        self.mlp_head_featbased = nn.Sequential(nn.LayerNorm(768), nn.Linear(768, L))


class _Tail(nn.Module):
    def __init__(self):
        super().__init__()
        with torch.device("meta"):   # shapes only: the last Linear alone is 537 MB
            self.emo_enc, self.sty_enc = _Heads(8), _Heads(30)
            self.fusion = _Fusion(768, 512)
            self.decode = _Decoder(512, 1024 * 128)


def _header():
    return re.sub(r"/\*.*?\*/", "", (REPO / "include/amuse_hip.h").read_text(), flags=re.S)


def test_spec_is_the_state_dict_of_stock_torch_modules_and_the_header_count():
    from amuse_amd import audio_weights as aw
    spec = aw.ast_tail_param_spec()
    sd = _Tail().state_dict()
    assert list(spec) == list(sd), [k for k in sd if k not in spec][:5]
    for k, shape in spec.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    total = aw.ast_tail_param_count()
    assert total == N_TAIL == sum(int(np.prod(s)) for s in spec.values())
    per768 = sum(int(np.prod(s)) for k, s in spec.items() if k.startswith("fusion.layers.0."))
    per512 = sum(int(np.prod(s)) for k, s in spec.items() if k.startswith("decode.layers.0."))
    heads = sum(int(np.prod(s)) for k, s in spec.items() if "_enc." in k)
    assert (per768, per512, heads) == (5513984, 3152384, 43084)
    assert int(re.search(r"#define AMUSE_AST_TAIL_PARAMS (\d+)u", _header()).group(1)) == total


def test_tail_weights_are_deterministic_and_the_big_matrix_has_no_equal_rows():
    from amuse_amd import audio_weights as aw
    w = aw.make_ast_tail_weights(3)
    assert list(w) == list(aw.ast_tail_param_spec()) and all(v.dtype == np.float32 and v.shape == aw.ast_tail_param_spec()[k] for k, v in w.items())
    W = w["decode.projection.2.weight"]
    # rows j + 1024 m share block row j: their ratio to row j is the per-row scale (0.5 .. 1.5 in magnitude, either sign), distinct among the 128 of them
    scale = W[:, 0].reshape(128, 1024).astype(np.float64) / W[:1024, 0][None, :]
    assert bool(np.isfinite(scale).all()) and 1 / 3.01 < float(np.abs(scale).min()) and float(np.abs(scale).max()) < 3.01
    assert all(len(np.unique(scale[:, j])) == 128 for j in range(1024)) and bool((scale < 0).any()) and bool((scale[1:] > 0).any())
    assert len(np.unique(W[:1024, :2], axis=0)) == 1024          # ... and the block's own rows differ
    assert 0.015 < float(W.std()) < 0.06 and abs(float(w["decode.norm.weight"].mean()) - 1.0) < 0.05
    again = aw.make_ast_tail_weights(3)
    assert all(np.array_equal(w[k], again[k]) for k in ("fusion.layers.1.linear1.weight", "emo_enc.mlp_head.1.bias"))
    assert np.array_equal(W[77777], again["decode.projection.2.weight"][77777])
    assert not np.array_equal(aw.make_ast_tail_weights(4)["fusion.fc.weight"], w["fusion.fc.weight"])


# ------------------------------------------------------------------------------------------------ the C ABI
NEW = ["amuse_audio_set_tail", "amuse_audio_encode_labels", "amuse_audio_reconstruct", "amuse_debug_tail_gemm", "amuse_debug_tail_pack"]


def test_header_declares_and_library_exports_the_tail():
    from amuse_amd import _lib
    hdr = _header()
    assert re.search(r"\bint\s+amuse_audio_set_tail\s*\(\s*amuse_audio_ctx\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)\s*;", hdr)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert int(re.search(r"#define AMUSE_ABI_VERSION (\d+)", hdr).group(1)) == 5 == _lib.ABI_VERSION
    lib = _lib.load()
    assert lib.amuse_abi_version() == 5
    assert set(NEW) <= set(_lib.EXPORTS)
    for name in NEW + ["amuse_audio_tail_ops"]:     # the full library carries the tail's translation unit
        assert hasattr(lib, name), name
    # _lib.EXPORTS follows the header: every amuse_* function it declares
    declared = set(re.findall(r"\b(amuse_\w+)\s*\(", hdr))
    assert declared <= set(_lib.EXPORTS) | {"amuse_audio_tail_ops"}, declared - set(_lib.EXPORTS)


def test_null_arguments_are_refused_without_touching_a_gpu():
    from amuse_amd import _lib
    lib = _lib.load()
    x = np.zeros(64, np.float32)
    p = x.ctypes.data_as(C.c_void_p)
    assert lib.amuse_audio_set_tail(None, p, N_TAIL) == -1
    assert lib.amuse_audio_encode_labels(None, 1, -1, p, 1, p, None, None) == -1
    assert lib.amuse_audio_reconstruct(None, p, p, p, 1, 1, p, None) == -1
    assert b"NULL" in lib.amuse_last_error()
    assert lib.amuse_debug_tail_gemm(None, p, p, 1, 256, 64, 1, p, None) == -1
    for N, K, prec in ((128, 64, 1), (256, 32, 1), (256, 96, 1), (256, 2048, 1), (256, 64, 0), (256, 64, 3)):
        assert lib.amuse_debug_tail_gemm(p, p, p, 1, N, K, prec, p, None) == -1, (N, K, prec)      # checked before any launch
        assert lib.amuse_debug_tail_pack(p, N, K, prec, p) == -1, (N, K, prec)
    assert lib.amuse_debug_tail_gemm(p, p, p, 0, 256, 64, 1, p, None) == -1


def _f16_split(w):
    hi = w.astype(np.float16)
    lo = (w - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


@pytest.mark.parametrize("N,K", [(256, 64), (512, 160 * 2)])
def test_pack_is_the_documented_permutation_and_rounding(N, K):
    from amuse_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(N + K)
    W = (rng.standard_normal((N, K)) * np.exp(rng.uniform(-12, 3, (N, K)))).astype(np.float32)   # magnitudes down into fp16's subnormals
    f, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    lane_term = ((((k & 31) >> 3) << 4) + (f & 15)) * 8 + (k & 7)
    unit = (f >> 4) * (K >> 5) + (k >> 5)
    # bf16: round to nearest even
    out = np.full(N * K, 0xdead, np.uint16)
    assert lib.amuse_debug_tail_pack(W.ctypes.data_as(C.c_void_p), N, K, _lib.PREC_BF16, out.ctypes.data_as(C.c_void_p)) == 0
    want = torch.from_numpy(W).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(out[unit * 512 + lane_term], want)
    assert len(np.unique(unit * 512 + lane_term)) == N * K          # a permutation: every slot written once
    # fp32x: hi unit, then lo unit - the bits of amuse_debug_f16_split
    outx = np.full(2 * N * K, 0xdead, np.uint16)
    assert lib.amuse_debug_tail_pack(W.ctypes.data_as(C.c_void_p), N, K, _lib.PREC_F32X, outx.ctypes.data_as(C.c_void_p)) == 0
    hi, lo = np.empty(N * K, np.uint16), np.empty(N * K, np.uint16)
    assert lib.amuse_debug_f16_split(W.ctypes.data_as(C.POINTER(C.c_float)), N * K, hi.ctypes.data_as(C.POINTER(C.c_uint16)), lo.ctypes.data_as(C.POINTER(C.c_uint16))) == 0
    nh, nl = _f16_split(W)
    assert np.array_equal(hi.reshape(N, K), nh) and np.array_equal(lo.reshape(N, K), nl)
    assert np.array_equal(outx[unit * 1024 + lane_term], nh) and np.array_equal(outx[unit * 1024 + 512 + lane_term], nl)
    # a feature tile's units are consecutive: features 16 .. 31 occupy exactly the second run of K / 32 units
    assert set((unit[16:32] // 1).ravel()) == set(range(K // 32, 2 * (K // 32)))


# ------------------------------------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip_with_and_without_a_tail(tmp_path, monkeypatch):
    from amuse_amd import audio_weights as aw
    from amuse_amd import checkpoint as ckpt
    tiny = OrderedDict([("v.cls_token", (1, 1, 4)), ("feature_head.1.weight", (2, 4))])
    tiny_tail = OrderedDict([("emo_enc.mlp_head.1.weight", (8, 4)), ("fusion.layers.0.self_attn.in_proj_weight", (12, 4)), ("decode.projection.2.bias", (6,))])
    monkeypatch.setattr(aw, "ast_param_spec", lambda: tiny)
    monkeypatch.setattr(aw, "ast_tail_param_spec", lambda: tiny_tail)
    sds = {e: {k: np.full(s, i, np.float32) for k, s in tiny.items()} for i, e in enumerate(aw.ENCODERS)}
    tail = {k: np.arange(int(np.prod(s)), dtype=np.float32).reshape(s) + j for j, (k, s) in enumerate(tiny_tail.items())}
    # without: the file of today, and no tail to load
    plain = ckpt.save_ast_reference_format(tmp_path / "plain", sds)
    assert set(torch.load(plain, weights_only=False)) == {f"{e}_enc.{k}" for e in aw.ENCODERS for k in tiny}
    assert ckpt.load_ast_tail(plain) is None
    assert float(ckpt.load_ast_checkpoint(plain)["sty"]["v.cls_token"].max()) == 2.0
    # with: the reference's names, un-prefixed, beside the encoders'
    full = ckpt.save_ast_reference_format(tmp_path / "full", sds, tail=tail)
    assert set(torch.load(full, weights_only=False)) == {f"{e}_enc.{k}" for e in aw.ENCODERS for k in tiny} | set(tiny_tail)
    back = ckpt.load_ast_tail(full)
    assert list(back) == list(tiny_tail) and all(np.array_equal(back[k], tail[k]) and back[k].dtype == np.float32 for k in tail)
    assert set(ckpt.load_ast_checkpoint(full)) == {"con", "emo", "sty"}
    # a file with SOME of the tail is an error, not an encoders-only file
    sd = torch.load(full, weights_only=False)
    del sd["decode.projection.2.bias"]
    torch.save(sd, full)
    with pytest.raises(KeyError):
        ckpt.load_ast_tail(full)


# ------------------------------------------------------------------------------------------------ collect_audio_metrics
REFERENCE_KEYS = {"fbanks", "emo", "sty", "con", "new_emo", "new_sty", "new_con"}     # AST_EVP.eval_func(metrics=True), AST_EVP.py:95-103


class _FakeEngine:
    has_tail = True

    def __init__(self):
        self.calls = []

    def fbank(self, waves):
        self.calls.append(("fbank", tuple(waves.shape)))
        return torch.zeros(waves.shape[0], 1024, 128)

    def metrics(self, fb):
        self.calls.append(("metrics", tuple(fb.shape)))
        d = {"fbanks": torch.ones(1024, 128)}
        for k, L in (("emo", 8), ("sty", 30), ("con", None)):
            for pre in ("", "new_"):
                d[pre + k] = {"feature": torch.full((256,), 2.0), "predicted_labels": None if L is None else torch.zeros(1, L)}
        return d


def test_collect_audio_metrics_writes_the_reference_pickle(tmp_path):
    from amuse_amd.infer_ldm import PretrainedLPDM_v1
    m = PretrainedLPDM_v1(None)
    with pytest.raises(NotImplementedError):
        m.collect_audio_metrics(torch.zeros(2, 1000), tgtpath=tmp_path)          # no engine
    m.audio_engine = _FakeEngine()
    m.audio_engine.has_tail = False
    with pytest.raises(NotImplementedError):
        m.collect_audio_metrics(torch.zeros(2, 1000), tgtpath=tmp_path)          # an engine without the tail
    m.audio_engine.has_tail = True
    m.collect_audio_metrics(torch.zeros(2, 1000), framerate=16000, baseline=False, tgtpath=tmp_path / "seq")
    assert m.audio_engine.calls == [("fbank", (1, 1000)), ("metrics", (1, 1024, 128))]   # channel 0, one clip
    with open(tmp_path / "seq" / "audio_metrics" / "fbank.pkl", "rb") as f:
        d = pickle.load(f)
    assert set(d) == REFERENCE_KEYS and d["fbanks"].shape == (1024, 128) and d["fbanks"].device.type == "cpu"
    for k in REFERENCE_KEYS - {"fbanks"}:
        assert set(d[k]) == {"feature", "predicted_labels"} and d[k]["feature"].shape == (256,)
    assert d["con"]["predicted_labels"] is None and d["new_con"]["predicted_labels"] is None
    assert d["emo"]["predicted_labels"].shape == (1, 8) and d["new_sty"]["predicted_labels"].shape == (1, 30)


def test_cli_flag_is_opt_in():
    src = (REPO / "amuse_amd" / "main.py").read_text()
    assert re.search(r'add_argument\("--audio-metrics",\s*action="store_true"', src)


# ------------------------------------------------------------------------------------------------ the host code under ASan / UBSan
@pytest.fixture(scope="module")
def host_tail_build(tmp_path_factory):
    import shutil
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("host_tail")
    build = subprocess.run(["bash", str(REPO / "tests" / "host_tail" / "build.sh"), str(out)], capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]
    return out


@pytest.mark.parametrize("prog,banner", [("host_tail", "AUDIO TAIL STUB OK\n"), ("host_notail", "AUDIO TAIL STUB OK (tail not linked)\n")])
def test_host_code_on_the_stubbed_runtime(host_tail_build, prog, banner):
    """host_tail: every EINVAL / ESTATE path (nothing allocated, nothing launched), then set_tail twice, reconstruct over one and two passes, encode_labels in the
    three pooling choices, destroy with no live allocation left.  host_notail: the link of tests/host_asan/build.sh - amuse_audio_api.o holds only a weak
    reference to the tail, so it links without amuse_audio_tail.o and every call that needs the tail returns AMUSE_ESTATE."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(host_tail_build / prog)], capture_output=True, text=True, timeout=900, env=env, cwd=str(host_tail_build))
    assert run.returncode == 0 and run.stdout.endswith(banner), run.stdout[-3000:] + run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
