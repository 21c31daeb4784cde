"""CPU (cross-compile only): the linear smoother's kernels (csrc/mht_smooth.hip: smooth_rts_kernel<NX, COV>, NX = 4 and 6, with and without
the covariance recursion) in both code objects; tests/test_smooth_ct_resources.py and test_smooth_ais_resources.py hold the file's other
kernels to the same (_report, _check_instances).  One track per lane with every matrix in registers: the six-state covariance kernel keeps
Pf, A Pf, the Cholesky factor, G and Ps - Pp live in one backward step and takes most of a lane's 512-entry register file (the compiler
parks part of it in the accumulator half).  What must not happen is a spill: scratch is 0 B with fully unrolled, statically indexed
matrices, and a later change that makes them spill or index dynamically is seen here.  Figures as read from the compiled objects."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pymht_amd", "csrc")

# instance -> (VGPRs, AGPRs) the compiler reports (identical in the two builds: the kernels do not depend on MHT_NX); the assertion is
# "no more than this", plus: no scratch, no spill, no LDS, and VGPRs + AGPRs within the 512 entries one wavefront per SIMD can have
READ = {
    "smooth_rts_kernelILi4ELb1E": (203, 0),
    "smooth_rts_kernelILi4ELb0E": (131, 0),
    "smooth_rts_kernelILi6ELb1E": (256, 144),
    "smooth_rts_kernelILi6ELb0E": (251, 0),
}


def _report(tmp_path, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from pymht_amd.build import FLAGS, SOURCES
    assert "mht_smooth.hip" in SOURCES, "the smoother is not part of the library"
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [hipcc] + flags + list(extra) + ["-c", "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"),
                                           os.path.join(CSRC, "mht_smooth.hip"), "-o", str(tmp_path / "o.o")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stderr
    found = {}
    num = lambda seg, pat: int(re.search(pat, seg).group(1))
    for m in re.finditer(r"Function Name: (\S+)", text):
        seg = text[m.end():m.end() + 4000]
        nxt = seg.find("Function Name:")
        seg = seg if nxt < 0 else seg[:nxt]
        found[m.group(1)] = dict(scratch=num(seg, r"ScratchSize \[bytes/lane\]: (\d+)"), vgpr=num(seg, r" VGPRs: (\d+)"), agpr=num(seg, r"AGPRs: (\d+)"),
                                 spill=num(seg, r"VGPRs Spill: (\d+)"), sgpr_spill=num(seg, r"SGPRs Spill: (\d+)"), lds=num(seg, r"LDS Size \[bytes/block\]: (\d+)"))
    return found


def _check_instances(found, read, build_nx):
    """What every smoother kernel is held to: exactly one instance per name in `read`, no VGPR spill, no scratch, no LDS, no more VGPRs and
    AGPRs than `read` says, and their sum within the 512 entries one wavefront per SIMD can have."""
    for kern, (vgpr, agpr) in read.items():
        hits = [(k, v) for k, v in found.items() if kern in k]
        assert len(hits) == 1, "kernel %s: %d instances in the compiler report of mht_smooth.hip (%d-state build)" % (kern, len(hits), build_nx)
        name, r = hits[0]
        print(name, r)
        # (SGPR "spills" are not asserted: the model's 72 float64 entries are wave-uniform kernel arguments, more than the 102 scalar
        # registers hold, and the compiler parks some in lanes of a vector register -- v_writelane / v_readlane, no memory behind it,
        # which the scratch figure below confirms)
        assert r["spill"] == 0, "%s spills %d VGPRs" % (name, r["spill"])
        assert r["scratch"] == 0, "%s uses %d B of scratch per lane: a matrix is indexed dynamically or registers spill" % (name, r["scratch"])
        assert r["lds"] == 0, "%s uses %d B of LDS" % (name, r["lds"])
        assert r["vgpr"] <= vgpr and r["agpr"] <= agpr, "%s needs %d VGPRs + %d AGPRs (read when written: %d + %d)" % (name, r["vgpr"], r["agpr"], vgpr, agpr)
        assert r["vgpr"] + r["agpr"] <= 512


@pytest.mark.parametrize("build_nx", [4, 6])
def test_smoother_kernels_do_not_spill(build_nx, tmp_path):
    _check_instances(_report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else []), READ, build_nx)


def test_smoother_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    assert "mht_smooth_tracks" in names and "mht_smooth_work_bytes" in names
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert hasattr(lib, "mht_smooth_tracks") and hasattr(lib, "mht_smooth_work_bytes"), "the %d-state build does not export the smoother" % nx
        # (pure host arithmetic, no GPU: the filtered mean and packed covariance of every node, plus the lengths)
        assert lib.mht_smooth_work_bytes(6, 2000, 400) == 8192 + 400 * (6 + 21) * 2000 * 8
        assert lib.mht_smooth_work_bytes(4, 3, 5) == 256 + 5 * (4 + 10) * 3 * 8
        assert lib.mht_smooth_work_bytes(5, 3, 5) == 0 and lib.mht_smooth_work_bytes(4, -1, 5) == 0


def test_constant_turn_model_is_refused_before_anything_runs():
    from pymht_amd.models import ct
    from pymht_amd.smoothing import smooth_tracks
    import numpy as np
    with pytest.raises(NotImplementedError, match="ct"):
        smooth_tracks(ct, 2.5, [(np.zeros(6), ct.P0, [None, np.zeros(2)])])


def test_reference_recursion_is_self_consistent():
    """tests/smooth_ref.py in float64 against itself in np.longdouble, and the textbook properties (the yardstick of test_smooth_gpu.py)."""
    import numpy as np
    import smooth_ref as sr
    from pymht_amd.models import ca
    assert np.finfo(np.longdouble).eps < 1e-18
    mats = sr.model_matrices(ca, 2.5)
    (x0, P0, z), = sr.make_batch(ca, 2.5, [60], seed=3)
    a, b = sr.rts(*mats, x0, P0, z, dtype=np.float64), sr.rts(*mats, x0, P0, z, dtype=np.longdouble)
    assert b["xs"].dtype == np.longdouble and 0 < sr.err(a["xs"], b["xs"]) < 1e-9 and sr.err(a["Ps"], b["Ps"]) < 1e-9
    assert np.array_equal(a["xs"][-1], a["xf"][-1]) and np.array_equal(a["xs"][0] != x0, np.ones(6, bool))
    tr = lambda M: np.trace(M, axis1=1, axis2=2)
    assert np.all(tr(a["Ps"]) <= tr(a["Pf"]) * (1 + 1e-9))
    one = sr.rts(*mats, x0, P0, z[:1])
    assert np.array_equal(one["xs"][0], x0) and np.array_equal(one["Ps"][0], P0)
