"""The host's arithmetic on a call's device clock stamps (csrc/pct_stamp.h): tests/host/stamp_host_check.cpp is a
stand-alone program with its own main and its own expectations; here it is compiled with the address and undefined-behaviour
sanitizers and run directly."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-cloud-toolbox_amd", "csrc")


def test_stamp_host_check(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "stamp_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "stamp_host_check.cpp"), "-o", str(exe), "-lm"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "stamp_host_check ok" in r.stdout
