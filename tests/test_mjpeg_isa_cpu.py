"""CPU: the resources of the preview video encoder's five kernels (csrc/k_mjpeg.hip) as hipcc states them in the gfx950 code object's metadata, from the
committed source: no spills and NO scratch at all (no per-lane array is indexed at run time), LDS = what the source declares, and register counts that keep
several waves per SIMD (recorded below).  A resource check only: the instructions are not read."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# what hipcc emitted when the kernels were written; the assertions below are the bounds
VGPRS_RECORDED = {"k_mjpeg_transform": 40, "k_mjpeg_size": 46, "k_mjpeg_scan_intervals": 18, "k_mjpeg_scan_frames": 22, "k_mjpeg_write": 37}
HUFF_WORDS = 2 * 256 + 2 * 16          # kMjpegHuffWords: AC luma, AC chroma, DC luma, DC chroma
# the source's __shared__ declarations: the DCT matrix + two [4 MCUs][3][64] float stages; the Huffman words; one scan array of 256 (32 bit | 64 bit)
LDS_DECLARED = {"k_mjpeg_transform": (64 + 2 * 4 * 3 * 64) * 4, "k_mjpeg_size": HUFF_WORDS * 4, "k_mjpeg_scan_intervals": 256 * 4, "k_mjpeg_scan_frames": 256 * 8,
                "k_mjpeg_write": HUFF_WORDS * 4}


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_mjpeg_kernels_registers_lds_and_no_scratch():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", "-", "k_mjpeg.hip"],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         out.stdout):
        ks[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgprs=int(m.group(4)), spills=int(m.group(5)))
    assert len(ks) == len(VGPRS_RECORDED), sorted(ks)
    src = (CSRC / "k_mjpeg.hip").read_text() + (CSRC / "amuse_mjpeg_host.hpp").read_text()
    assert "kMjpegHuffWords = 2 * 256 + 2 * 16" in src and "kMjpegScanBlock = 256" in src and "kMjpegTransformMcus = 4" in src      # the constants LDS_DECLARED restates
    for short in VGPRS_RECORDED:
        k = next(v for n, v in ks.items() if short + "E" in n)
        print(f"{short}: {k['vgprs']} VGPRs (recorded {VGPRS_RECORDED[short]}), scratch {k['scratch']}, spills {k['spills']}, LDS {k['lds']}")
        assert k["spills"] == 0 and k["scratch"] == 0 and k["lds"] == LDS_DECLARED[short] and k["vgprs"] <= 128, (short, k)
