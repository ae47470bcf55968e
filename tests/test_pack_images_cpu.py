"""CPU: every byte the weight packers upload, every stage / unit table the launchers are handed and every device re-pack, for the four Denoiser archs, against
tests/golden/pack_images.json.  tests/host_asan/pack_images.cpp drives the library's host code through the C ABI on the stubbed HIP runtime, whose image log
(tests/host_asan/hip_stub.cpp) prints sizes and 64-bit FNV-1a digests; the log is compared section by section (one section per ABI call group), as a multiset
inside a section (the order of uploads inside one build is not part of the contract; the bytes are).

The golden file was recorded ONCE, with this driver and stub, from the commit BEFORE the packers were gathered into amuse_pack.hpp (the copy-and-paste builders
of amuse_api.hip / amuse_variants.hip): `tests/host_asan/build.sh DIR && DIR/pack_images > LOG && python tests/test_pack_images_cpu.py LOG`.  It states what the
kernels consume; it is never regenerated from refactored packing code - a packer that changes a kernel's weight order changes the kernel with it and says so.

One image is not a function of the parameters alone: den_freqs (128 floats from expf / logf on the host; 512 bytes, first element exactly 1.0f - no parameter
image starts with 1.0f, the LCG's values lie in [-0.1, 0.1]).  libm may round it differently on another machine, so its digest is left out of the golden: the
FIRST such upload of a context is skipped, every later one of that context must repeat it bit for bit, and nothing else is skipped."""
import json
import os
import re
import subprocess
import sys
from collections import Counter
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden" / "pack_images.json"
FREQS = re.compile(r"^upload bytes=512 digest=([0-9a-f]{16}) first=3f800000$")
ELEM_BYTES = {0: 4, 1: 2, 2: 2, 3: 2}        # launch_repack's kind: fp32 | bf16 | split-fp16 | fp16
KIND_OF_BIT = {1: 0, 2: 1, 8: 2, 16: 3}      # AMUSE_UPD_F32 | _BF16 | _F32X | _F16 -> the kind of that precision's streams
ENCODER = 4                                  # AMUSE_UPD_ENCODER


def sections_of(text):
    """[(name, [lines])] of a driver log; den_freqs uploads are taken out and returned per context as [digests]."""
    secs, freqs = [], {}
    for line in text.splitlines():
        if line.startswith("== "):
            secs.append((line[3:], []))
            continue
        if not secs or line == "PACK IMAGES OK":
            continue
        m = FREQS.match(line)
        if m:
            freqs.setdefault(secs[-1][0].split(" ")[1], []).append(m.group(1))
            continue
        secs[-1][1].append(line)
    return secs, freqs


def to_golden(text):
    secs, _ = sections_of(text)
    return {"sections": [[name, dict(sorted(Counter(lines).items()))] for name, lines in secs]}


def test_packed_images_stage_tables_and_repack_maps_match_the_golden(host_asan_build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(host_asan_build / "pack_images")], capture_output=True, text=True, timeout=900, env=env)
    assert run.returncode == 0 and "PACK IMAGES OK" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    secs, freqs = sections_of(run.stdout)
    golden = json.loads(GOLDEN.read_text())["sections"]
    assert [name for name, _ in secs] == [name for name, _ in golden]
    assert len({name for name, _ in secs}) == len(secs)
    for (name, lines), (_, want) in zip(secs, golden):
        got = Counter(lines)
        missing, extra = Counter(want) - got, got - Counter(want)
        assert not missing and not extra, f"section '{name}': missing {dict(missing)}, unexpected {dict(extra)}"
    # the one exclusion: one free digest per context, every later upload of den_freqs in that context repeats it
    assert len(freqs) <= 4 and all(arch in "0123" for arch in freqs)   # at most one skipped entry per context
    for arch, digests in freqs.items():
        assert all(d == digests[0] for d in digests[1:]), f"arch {arch}: den_freqs changed between uploads"
    n_lines = sum(len(lines) for _, lines in secs)
    assert n_lines == sum(sum(want.values()) for _, want in golden) and n_lines > 3000

    # amuse_update_weights_device re-packs exactly the images amuse_update_weights re-uploads for the same mask: the same count, the same element counts, the
    # same kinds.  Images that every mask re-uploads are the small fp32 parameters (kind 0); what a mask adds to them are its precision's streams.
    by_name = dict(secs)
    masks = [bit | enc for bit in KIND_OF_BIT for enc in (0, ENCODER)]
    uploads = {}
    for what in masks:
        sizes = Counter()
        for line in by_name[f"arch 0 update what={what}"]:
            m = re.match(r"^upload bytes=(\d+) ", line)
            assert m, line
            sizes[int(m.group(1))] += 1
        uploads[what] = sizes
    always = uploads[masks[0]]
    for what in masks[1:]:
        always = always & uploads[what]
    assert sum(always.values()) > 20
    for what in masks:
        want = Counter()
        for size, n in uploads[what].items():
            small = min(n, always[size])
            if small:
                want[(size // 4, 0)] += small
            if n - small:
                kind = KIND_OF_BIT[what & ~ENCODER]
                want[(size // ELEM_BYTES[kind], kind)] += n - small
        got = Counter()
        for line in by_name[f"arch 0 device what={what}"]:
            m = re.match(r"^launch_repack n=(\d+) kind=(\d) image=([0-9a-f]{16}) ", line)
            assert m, line
            assert m.group(3) != "0" * 16, "a re-pack into memory that no upload ever filled"
            got[(int(m.group(1)), int(m.group(2)))] += 1
        assert got == want, f"mask {what}: device re-pack {dict(got)} against host re-upload {dict(want)}"


if __name__ == "__main__":   # record: see the module docstring
    GOLDEN.write_text(json.dumps(to_golden(Path(sys.argv[1]).read_text()), indent=0, separators=(",", ":")) + "\n")
