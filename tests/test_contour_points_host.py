"""lg_host_contour_points (csrc/lg_contour.cpp: the trace behind lg_leaf_contour and _get_edge_points) against the
oracle's independent trace (oracle/lg_oracle.c), point for point in tracing order.  The product code is built into a
stand-alone program with g++ -fsanitize=address,undefined and run once over all masks: a sanitizer report fails the
test.  No GPU involved, nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from oracle import lg_oracle as O
from tests import collector_cases as CC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "leaf-grasping-vision-ml_amd", "csrc")

DRIVER = r'''
// in : int32 count, then per mask int32 H, W and H*W bytes
// out: per mask int32 n and n (x, y) int32 pairs
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "lg_internal.h"
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 3;
    int32_t count = 0;
    if (fread(&count, 4, 1, fi) != 1) return 4;
    for (int i = 0; i < count; i++) {
        int32_t hw[2];
        if (fread(hw, 4, 2, fi) != 2) return 5;
        const int H = hw[0], W = hw[1], WW = (W + 63) / 64;
        std::vector<uint8_t> m((size_t)H * W);
        if (fread(m.data(), 1, m.size(), fi) != m.size()) return 6;
        std::vector<unsigned long long> bits((size_t)H * WW, 0ull);   // exactly H * WW words: a read past them is reported
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                if (m[(size_t)y * W + x]) bits[(size_t)y * WW + (x >> 6)] |= 1ull << (x & 63);
        std::vector<int> xy;
        const int32_t n = lg_host_contour_points(bits.data(), H, W, WW, xy);
        if ((size_t)n * 2 != xy.size()) return 7;
        fwrite(&n, 4, 1, fo);
        if (n) fwrite(xy.data(), 4, xy.size(), fo);
    }
    fclose(fi);
    return fclose(fo) ? 8 : 0;
}
'''


def _cases():
    ms = [(f"random{i}", m) for i, m in enumerate(CC.random_contour_masks())]
    for H, W in ((33, 47), (64, 96), (67, 130)):   # single pixel, line, equal pair, area-0 components, full, comb, ...
        ms += [(f"{k}@{H}x{W}", m) for k, m in CC.contour_masks(H, W).items()]
    ms.append(("one_pixel_frame", np.ones((1, 1), np.uint8)))
    ms.append(("row", np.ones((1, 70), np.uint8)))
    ms.append(("column", np.ones((70, 1), np.uint8)))
    ms.append(("word_edge", np.pad(np.ones((3, 2), np.uint8), ((2, 2), (63, 63)))))   # a blob on columns 63 | 64
    return ms


def test_host_contour_points_match_oracle_under_sanitizers(tmp_path):
    src = tmp_path / "driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "contour_points"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
                           str(src), os.path.join(CSRC, "lg_contour.cpp"), "-o", str(exe)])
    cases = _cases()
    assert sum(n.startswith("random") for n, _ in cases) == 120
    fin, fout = tmp_path / "masks.bin", tmp_path / "points.bin"
    with open(fin, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for _, m in cases:
            f.write(np.array(m.shape, np.int32).tobytes())
            f.write(np.ascontiguousarray(m, dtype=np.uint8).tobytes())
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = np.fromfile(fout, np.int32)
    pos, nonempty, multi = 0, 0, 0
    for name, m in cases:
        n = int(got[pos])
        pts = got[pos + 1:pos + 1 + 2 * n].reshape(n, 2)
        pos += 1 + 2 * n
        exp = O.leaf_contour_points(m)
        assert n == len(exp), name
        np.testing.assert_array_equal(pts, exp, err_msg=name)
        nonempty += n > 0
        multi += n > 1
    assert pos == len(got) and nonempty > 100 and multi > 80
