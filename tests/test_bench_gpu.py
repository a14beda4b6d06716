"""bench.py's two shapes on a small flightline: a plain run prints the headline alone, --full adds the sections that take runs
of their own (here: the one-in-flight pass and the score kernel's roofline; the others need the full-size cube or a host minute)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--lines", "1200", "--samples", "40"]
HEADLINE = {"metric": "CMF Mpixels/s on 598x20000x425 cube", "unit": "Mpixel/s", "higher_is_better": True, "dtype": "f64"}


def _line(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k, v in HEADLINE.items():
        assert line[k] == v
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    assert abs(line["value"] - 1200 * 40 / (line["ms_per_step"] * 1e-3) / 1e6) <= 1e-2 * line["value"]
    return line


def test_plain_run_prints_the_headline_alone():
    line = _line([])
    assert "one_in_flight" not in line["config"] and "one_in_flight" not in line["config"]["product_buffer_placement"]
    for k in ("roofline", "cpu_baseline", "cnn", "e2e", "co2", "reflectance", "wide", "ingest", "sweep_routes", "hard_spectrum"):
        assert k not in line
    # the --no-* options of the full run are accepted and change nothing here
    assert set(_line(["--no-cpu-baseline", "--no-cnn"])) == set(line)


def test_full_run_adds_the_one_in_flight_pass_and_the_roofline():
    line = _line(["--full", "--no-cpu-baseline", "--no-cnn"])
    assert line["config"]["one_in_flight"]["ms_per_step"] > 0
    assert "one_in_flight" in line["config"]["product_buffer_placement"]
    assert line["roofline"]["avg_launch_ms"] > 0 and line["roofline"]["launches"] == 2


def test_a_run_with_one_flightline_in_flight_has_its_roofline_without_full():
    line = _line(["--in-flight", "1"])
    assert line["roofline"]["avg_launch_ms"] > 0 and line["config"]["one_in_flight"]["ms_per_step"] == line["ms_per_step"]
