"""The outlier rule of csrc/b4d_keys.hpp (outlier_rhs, outlier_rejected: what b4d_despeckle applies over a window and
b4d_temporal_robust_mean along a stack), run as host code by a small C++ program over a grid of samples, medians, MADs and
settings, against the one NumPy model of the rule (tests/temporal_order_model.py: outlier_rule).  rhs is compared bit for bit
(NaN equal to NaN), the decision exactly."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import temporal_order_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RULE_PROGRAM = r"""
// Prints outlier_rhs and outlier_rejected of b4d_keys.hpp over the grid of the Python side, one row per combination:
// x med mad threshold min_scale (float bits), scale_kind, polarity, rhs (float bits), rejected.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "b4d_keys.hpp"
using namespace b4d::keys;

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float den = std::numeric_limits<float>::denorm_min();
    const float xs[10] = {-0.0f, 0.0f, den, 1.0f, std::nextafter(1.0f, 2.0f), 50.0f, 1e30f, inf, -inf, nan};
    const float mads[4] = {0.0f, den, 0.5f, nan};
    const float thresholds[3] = {0.0f, 3.0f, 5.0f};
    const float floors[2] = {0.0f, 1.0f};
    for (float x : xs)
        for (float med : xs)
            for (float mad : mads)
                for (float thr : thresholds)
                    for (float floor_ : floors)
                        for (int kind = 0; kind < 3; ++kind)
                            for (int pol = 0; pol < 3; ++pol) {
                                const OutlierRule r = make_outlier_rule(kind, thr, floor_, pol);
                                const float rhs = outlier_rhs(r, med, mad);
                                std::printf("%08x %08x %08x %08x %08x %d %d %08x %d\n", float_bits(x), float_bits(med), float_bits(mad),
                                            float_bits(thr), float_bits(floor_), kind, pol, float_bits(rhs),
                                            outlier_rejected(r, x, med, rhs) ? 1 : 0);
                            }
    return 0;
}
"""


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("outlier_rule")
    src, exe = d / "rule.cpp", d / "rule"
    src.write_text(RULE_PROGRAM)
    # a stand-alone program with its own main: the sanitizers are linked in the ordinary way
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "barc4dip_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:      # a compiler without the sanitizer runtimes still checks the rule
        r = subprocess.run([c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_outlier_rule_as_host_code(rule_program):
    """x, med in {-0, 0, denormal, 1, 1 + ulp, 50, 1e30, +Inf, -Inf, NaN}, mad in {0, denormal, 0.5, NaN}, threshold in {0, 3, 5},
    min_scale in {0, 1}, the three scales and the three polarities: 21600 rows."""
    r = subprocess.run([rule_program], capture_output=True, text=True, check=True)
    rows = np.array([[int(v, 16) for v in line.split()] for line in r.stdout.splitlines()], dtype=np.uint64)
    assert rows.shape == (10 * 10 * 4 * 3 * 2 * 3 * 3, 9)
    f32 = lambda col: rows[:, col].astype(np.uint32).view(np.float32)
    x, med, mad, thr, floor_ = (f32(c) for c in range(5))
    assert len(np.unique(rows[:, 0])) == 10 and len(np.unique(rows[:, 1])) == 10 and len(np.unique(rows[:, 2])) == 4
    kind, pol, got_rhs, got_rej = rows[:, 5], rows[:, 6], f32(7), rows[:, 8].astype(bool)
    seen = 0
    for t in (0.0, 3.0, 5.0):
        for fl in (0.0, 1.0):
            for k, scale in enumerate(M.SCALES):
                for p, polarity in enumerate(M.POLARITIES):
                    sel = (thr == np.float32(t)) & (floor_ == np.float32(fl)) & (kind == k) & (pol == p)
                    assert sel.sum() == 400
                    rhs, rej = M.outlier_rule(x[sel], med[sel], mad[sel], t, scale, polarity, fl)
                    same = (rhs.view(np.uint32) == got_rhs[sel].view(np.uint32)) | (np.isnan(rhs) & np.isnan(got_rhs[sel]))
                    assert same.all() and np.array_equal(rej, got_rej[sel]), (t, fl, scale, polarity)
                    assert rej.any() and not rej.all()
                    seen += int(sel.sum())
    assert seen == len(rows)
