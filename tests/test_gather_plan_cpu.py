"""CPU tests (no GPU, no RCCL) of the multi-GPU gather's bookkeeping (fm-radio_amd/csrc/fmd_gather_plan.h, the HIP-free half of
libfmdgather.so): who collects block k under FMD_GATHER_ROTATE, which shards cross RCCL and which are copies, the back-pressure on the
collector's three buffer sets, and that fmd_gather_abort's host side releases every waiter (reference anchor: one
demodulator wired to an audio observer and an RDS byte chain per station, src/app.cpp:19-34)."""
import json
import platform
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gather_plan") / "gather_plan_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'fm-radio_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "gather_plan_main.cpp"),
                    "-lpthread", "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("args", [["plan"], ["run", "2", "150"], ["run", "4", "300"], ["run", "8", "120"], ["abort"]])
def test_gather_bookkeeping(driver, args):
    r = subprocess.run([str(driver), *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["failed_checks"] == 0


@pytest.mark.parametrize("san,args", [("thread", ["run", "4", "100"]), ("thread", ["abort"]), ("address,undefined", ["plan"]), ("address,undefined", ["run", "3", "60"])])
def test_gather_bookkeeping_under_sanitizers(tmp_path, san, args):
    """The host-side hand-shake is lock-free (atomics between the rank threads and the collecting thread): ThreadSanitizer on the
    simulated runs, AddressSanitizer / UBSan on the plan logic (CPU builds only: the suite runs no sanitizer on GPU code)."""
    exe = tmp_path / "gather_plan_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", f"-fsanitize={san}", "-fno-sanitize-recover=all", f"-I{ROOT / 'fm-radio_amd' / 'csrc'}",
                    str(ROOT / "tests" / "cpp" / "gather_plan_main.cpp"), "-lpthread", "-o", str(exe)], check=True)
    # GCC's ThreadSanitizer runtime aborts ("unexpected memory mapping") where the kernel randomises mmap addresses more widely than
    # its shadow layout allows: the instrumented binary runs without address-space randomisation (a personality flag of that process only)
    no_aslr = [shutil.which("setarch"), platform.machine(), "-R"] if san == "thread" and shutil.which("setarch") else []
    r = subprocess.run([*no_aslr, str(exe), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stderr[-3000:], r.stdout[-500:])
    assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr
