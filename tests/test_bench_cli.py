"""bench.py's command line, without a GPU: the options a plain run and a --full run are asked for with, and the
combinations it refuses before it touches anything."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, capture_output=True,
                          text=True, timeout=120)


def test_help_names_full_and_dump_outputs():
    proc = _bench("--help")
    assert proc.returncode == 0 and "--full" in proc.stdout and "--dump-outputs" in proc.stdout


def test_steps_must_be_positive():
    proc = _bench("--steps", "0")
    assert proc.returncode == 2 and "--steps must be at least 1" in proc.stderr and "{" not in proc.stdout


def test_dump_outputs_is_for_the_integration_only(tmp_path):
    for extra in (["--rows"], ["--dry-run-dist"]):
        proc = _bench("--steps", "1", "--dump-outputs", str(tmp_path / "out"), *extra)
        assert proc.returncode == 2 and "--dump-outputs" in proc.stderr and "{" not in proc.stdout
    assert not (tmp_path / "out").exists()
