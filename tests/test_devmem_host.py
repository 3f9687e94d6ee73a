"""The bookkeeping of DevBufs and the context's buffer pool (csrc/fpm_devmem.cpp), checked by
fp-mash_amd/tools/devmem_check.cpp under the host address and undefined-behaviour sanitizers.
The program is built from the owner and the pool helpers alone and runs only where no device is
visible: every allocation fails there, and the addresses it hands the owner are made up."""
import os
import subprocess

import pytest

from conftest import ROOT

AMD = os.path.join(ROOT, "fp-mash_amd")
HIPCC = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")


def test_devbufs_bookkeeping(tmp_path):
    import fpmash
    if fpmash.device_count() > 0:
        pytest.skip("a device is visible")
    exe = str(tmp_path / "devmem_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall",
                    "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(AMD, "csrc", "fpm_devmem.cpp"),
                    os.path.join(AMD, "tools", "devmem_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "devmem ok", r.stdout + r.stderr
