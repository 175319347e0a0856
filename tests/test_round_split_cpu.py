"""Round split, host side: the generation arithmetic of gs_split_plan.h (no GPU)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_generations_under_host_sanitizers(tmp_path):
    """tests/split_plan_check.cpp: over 12 rounds with joins and resets at arbitrary points, the
    generation each round reads, the one its rotation writes, the lists its catch-up copy names,
    that no launch writes what a launch that may still run reads or writes under the event
    dependencies, and that a model of the rows driven by the plan equals a single buffer rotated
    in place. A stand-alone program with its own main, compiled with -fsanitize=address,undefined
    on the host compiler and run directly."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "split_plan_check")
    # (the sanitizer runtimes linked statically: the program needs nothing loaded before it)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gossip-sim_amd", "csrc"),
                    os.path.join(ROOT, "tests", "split_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
