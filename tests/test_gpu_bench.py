"""bench.py's two kinds of run on a small frame: a plain run prints the headline line without the CPU baseline and the parity
leg, `--full` adds both and the parity holds.  Each run is a fresh child process with a time limit; the test process itself
never opens the GPU, and once a run overruns its limit or dies by a signal nothing more is started."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

SMALL = ["--gpus", "1", "--steps", "1", "--warmup", "1", "--xres", "64", "--yres", "36", "--spp", "4"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(extra, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, "bench.py %s: exit %d\n%s" % (" ".join(extra), r.returncode, r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_full_adds_cpu_baseline_and_parity():
    plain = _bench([], timeout=180)
    for k in HEADLINE:
        assert k in plain, k
    assert plain["unit"] == "Msamples/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert "cpu_baseline" not in plain and "parity" not in plain
    assert plain["roofline"]["kernel_launches"] >= 1

    full = _bench(["--full"], timeout=300)
    for k in HEADLINE:
        assert k in full, k
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["unit"] == "Msamples/s"
    assert full["parity"]["ok"] and full["parity"]["rng_end_positions_equal"]
    assert full["parity_max_rel_l2"] <= 1e-4
    # same inputs, same frame: the timed steps compute what the plain run computed (up to the order of the film's float adds)
    assert abs(full["checksum"] - plain["checksum"]) <= 1e-5 * abs(plain["checksum"])
