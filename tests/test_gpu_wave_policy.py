"""The device's wave policy checked directly (tests/c/wave_policy_gpu.hip): one exerciser of ballots, sums, or64,
add64, lanes phases, one + sync loops and the lane-mask helpers, with the deciding lane on 0, 31/32 and 63, runs under
DevWave (one-wave blocks striding over work items, as the kernels do), under SerialWave inside a lane (the resend's
lane form) and under SerialWave on the host; the three outputs must be equal byte for byte and equal to values that
plain loops write down.  Then kernargs<Args>() for structs of FqArgs' and RsCommitArgs' sizes, every field echoed.
A stand-alone program run once as a child process; the test without the gpu mark only compiles it, so that it cannot
rot where there is no device."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "wave_policy_gpu.hip")


def build(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "wave_policy_gpu")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", SRC, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def test_wave_policy_program_compiles(tmp_path):
    assert os.path.getsize(build(tmp_path)) > 0


@pytest.mark.gpu
def test_wave_policy_on_the_device(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    # 3 forms x 100 items x 24 words, and the 16 + 32 echoed fields
    assert r.stdout.strip() == "ok: %d" % (3 * 100 * 24 + 16 + 32), r.stdout
