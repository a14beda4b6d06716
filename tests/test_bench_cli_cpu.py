"""bench.py's command line without a GPU: --full exists and is off by default, and the project's scripts that read sections
only a full run measures ask for one."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_is_an_option_of_the_benchmark():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout


def test_final_measure_asks_for_a_full_run_where_it_reads_the_roofline_of_a_depth_three_run():
    """tools/final_measure.sh asserts roofline.avg_launch_ms of every line it keeps: a run with three flightlines in flight has
    that figure only from the one-in-flight pass of --full."""
    runs = [l for l in open(os.path.join(ROOT, "tools", "final_measure.sh")) if re.match(r"\s*python3? bench\.py", l)]
    assert len(runs) == 3
    for l in runs:
        assert "--full" in l or "--in-flight 1" in l, l
