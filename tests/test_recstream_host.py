"""csrc/recstream_dev.h on the CPU: the index arithmetic both stream encoders place their records by (the copy-out's head / body / tail
ranges, the parts picker), compiled as a stand-alone program by the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer.
The checks themselves are in tests/recstream/recstream_host.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_copy_ranges_and_parts_picker_on_the_host(tmp_path):
    exe = str(tmp_path / "recstream_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "bs_call_amd", "csrc"),
                    os.path.join(ROOT, "tests", "recstream", "recstream_host.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:] + p.stderr[-3000:]
