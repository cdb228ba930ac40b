"""rbe_scratch.h, the host layer's owning buffer type, over a fake memory
policy: tests/scratch_cpu/scratch_cpu.cpp is a stand-alone program, built here
with the address and undefined-behaviour sanitizers and run (reuse without an
allocator call, free-before-allocate growth and its capacities, a refused
allocation, the kept prefix of reserve_keep, one free per buffer)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_scratch_cpu(tmp_path):
    exe = tmp_path / "scratch_cpu"
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(HERE, "scratch_cpu", "scratch_cpu.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("scratch_cpu ok"), out.stdout + out.stderr
