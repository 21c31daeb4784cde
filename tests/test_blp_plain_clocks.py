"""CPU (cross-compile only): the plain instance of the union-find ILP launch reads no phase clocks, counted in the compiler's own assembly
listing of mht_blp.hip (gfx950, the library's flags; the listing of tests/test_blp_clock_census.py).

blp_uf_kernel_plain keeps seven clock reads (s_memrealtime for the wall clock, s_memtime for the shader clock): the report's stage stamps
DevStatus::t[1], t[2] and t[4], a cluster's start and the read behind its records (cl_time column 1), and the time limit of the branch and
bound in its two storage policies.  The phase statistics -- the workgroup's first instruction, the set-up stamp, the shader clock, the
stamps of the dual phase and of the exact search -- are hidden from it by BlpArgsPlain::phase_clocks.  Scalar memory returns out of order:
a clock read in front of the prologue's first global_load is drained, clock latency included, before the parents' round trip may leave,
on every workgroup of the launch -- so none may stand there.  The generic instance blp_uf_kernel, which tools/blp_uf_profile.py and
tools/ilp_dist.py run, keeps every stamp."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pymht_amd", "csrc")

PLAIN_MAX = 7            # blp_uf_kernel_plain: see above (27 before the phase statistics were compiled out of it)
GENERIC_MIN = 39         # blp_uf_kernel: every stamp it had

CLOCK = re.compile(r"^\s*s_mem(?:real)?time\b")
GLOBAL_LOAD = re.compile(r"^\s*global_load")
INSTRUCTION = re.compile(r"^\s+[a-z]\w*")      # (labels start in column 0, directives with a dot, comments with a semicolon)


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
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
        found[m.group(1)] = [ln for ln in text[m.end():end].split("\n") if INSTRUCTION.match(ln)]
    generic = [v for k, v in found.items() if "plain" not in k]
    plain = [v for k, v in found.items() if "plain" in k]
    assert len(generic) == 1 and len(plain) == 1, sorted(found)
    return generic[0], plain[0]


def _clocks(instructions):
    return [i for i, ln in enumerate(instructions) if CLOCK.match(ln)]


def test_plain_instance_holds_at_most_seven_clock_reads(listing):
    _, plain = listing
    n = len(_clocks(plain))
    print("clock reads in blp_uf_kernel_plain: %d" % n)
    assert n <= PLAIN_MAX, n


def test_plain_instance_reads_no_clock_in_front_of_its_first_global_load(listing):
    _, plain = listing
    loads = [i for i, ln in enumerate(plain) if GLOBAL_LOAD.match(ln)]
    clocks = _clocks(plain)
    assert loads, "no global_load in the listing of blp_uf_kernel_plain"
    print("blp_uf_kernel_plain: first global_load is instruction %d, first clock read %s" % (loads[0], clocks[0] if clocks else "none"))
    assert not clocks or clocks[0] > loads[0], (clocks[0], loads[0])


def test_generic_instance_keeps_every_stamp(listing):
    generic, _ = listing
    n = len(_clocks(generic))
    print("clock reads in blp_uf_kernel: %d" % n)
    assert n >= GENERIC_MIN, n
