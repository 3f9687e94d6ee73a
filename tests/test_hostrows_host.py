"""The host's row packer (host/SketchRows.h) and number formatters (host/TextOut.h), checked by
fp-mash_amd/tools/hostrows_check.cpp under the host address and undefined-behaviour sanitizers:
the packer against a one-thread, per-hash loop (u64 and u32, empty and full rows, a minimum width,
no rows, 4097 rows for the threaded path), the formatters against snprintf and std::to_string.
The program is built from the two headers alone, needs no device, and like the devmem check
runs only where none is visible."""
import os
import subprocess

import pytest

from conftest import ROOT

AMD = os.path.join(ROOT, "fp-mash_amd")
HIPCC = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")


def test_hostrows_packer_and_formatters(tmp_path):
    import fpmash
    if fpmash.device_count() > 0:
        pytest.skip("a device is visible")
    exe = str(tmp_path / "hostrows_check")
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-Wall",
                    "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(AMD, "tools", "hostrows_check.cpp"), "-o", exe, "-lpthread"],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "hostrows ok", r.stdout + r.stderr
