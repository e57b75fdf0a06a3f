"""The closed-loop kernels' arguments without a GPU: tests/loop_args_check_main.cpp, a stand-alone program with its own main around the host
functions that build them (csrc/slsqp_api.hip compiled for the host only), built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_one_qp_args_per_chain_and_the_staged_block_under_sanitizers():
    """The two QpArgs of a chain filled independently (warm, stat_slot, snap_use) = (w, 0, 0) and (1, 1, 1) against the common struct and
    qp_second_args, memcmp, for w = 0 and 1; the block the host stages for a launch against what went to the kernels by value, field by field; a
    second launch of the same handle with other steps and options; the description of the handle's options (cl_options) in each of the 8 states of
    (reference, plant parameters, bounds): the kernels' variant and arguments, and the bounds in the block against the struct they were before; every
    argument builder against the positional initialiser it replaced, field by field, for each combination of its parameters a launch site uses, and
    make_chain_args / make_loop_block against the same composition written the old way, memcmp, plain and SCP in the option states 000 and 111; no
    launch entered by make_qp_args, make_chain_args or make_loop_block on handles that ask for a non-zero x0 tolerance; with_dims on a pair outside
    the build's list returns non-zero, does not call its function, and slsqp_last_error names the pair and the list."""
    exe = os.path.join(ROOT, "tests", "_build", "loop_args_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    # (host pass only: no device code is generated, so this is the host compiler's time; the sanitizer runtimes are linked into the program)
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-fuse-cuid=none", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Wno-pass-failed",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "loop_args_check_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "loop_args_check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
