"""CPU (cross-compile only): how often the two instances of the union-find ILP launch read the clock, counted in the compiler's own
assembly listing of mht_blp.hip (gfx950, the library's flags).

Scalar memory returns out of order, so every clock read (s_memrealtime for the wall clock, s_memtime for the shader clock) turns the next
LDS or scalar wait of the wavefront into a full lgkmcnt(0) drain with the clock's latency inside it -- on a workgroup that runs one
wavefront per SIMD and ends the scan's critical path.  Compiling the phase statistics out of the plain instance (7 reads left) was measured
at +1.2 % on the headline, less than five times the parent's run-to-run spread, and is not in the tree (profiles/ilp_prologue.txt): the
plain instance holds what it held, and this test keeps it from holding more.  The generic instance, which tools/ilp_dist.py and
tools/blp_uf_profile.py ask for, keeps every stamp."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pymht_amd", "csrc")

# clock reads in the listing, AMD clang 22.0.0git (roc-7.2.0, HIP 7.2.26015)
PARENT_PLAIN = 27        # blp_uf_kernel_plain at the parent commit
PARENT_GENERIC = 39      # blp_uf_kernel at the parent commit
PLAIN_MAX = 27           # blp_uf_kernel_plain now: unchanged

CLOCK = re.compile(r"^\s*s_mem(?:real)?time\b", re.M)


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from pymht_amd.build import FLAGS
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC")]
    asm = str(tmp_path_factory.mktemp("blp") / "mht_blp.s")
    out = subprocess.run([hipcc] + flags + ["-S", "--offload-device-only", "-I", os.path.join(ROOT, "include"),
                                            os.path.join(CSRC, "mht_blp.hip"), "-o", asm], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    text = open(asm).read()
    found = {}
    for m in re.finditer(r"^(_ZN3mht\w*blp_uf_kernel\w*):\s*(?:;.*)?$", text, re.M):
        end = text.find(".Lfunc_end", m.end())
        assert end > 0, m.group(1)
        found[m.group(1)] = len(CLOCK.findall(text[m.end():end]))
    generic = [v for k, v in found.items() if "plain" not in k]
    plain = [v for k, v in found.items() if "plain" in k]
    assert len(generic) == 1 and len(plain) == 1, sorted(found)
    print("clock reads: generic %d (parent %d), plain %d (parent %d)" % (generic[0], PARENT_GENERIC, plain[0], PARENT_PLAIN))
    return generic[0], plain[0]


def test_plain_instance_reads_the_clock_no_more_often_than_before(census):
    _, plain = census
    assert 2 <= plain <= PLAIN_MAX, plain       # (at least a cluster's start and its end: cl_time column 1)


def test_generic_instance_keeps_its_phase_statistics(census):
    generic, _ = census
    assert generic >= PARENT_GENERIC, generic
