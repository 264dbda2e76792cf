"""The weighted host sampler (csrc/neighbor_sample_host.cc and the key rule of
csrc/sample_key.h) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/c_client/weighted_sample_sanitize.c, a stand-alone C program linked with
the sanitized host library (`make -C dgl-1_amd/csrc asan`), drives
dglhip_neighbor_sample_host_weighted, dglhip_neighbor_sample_host_fetch, the
two key exports and the error paths. CPU only; nothing loaded into Python is
sanitized."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weighted_host_sampler_under_asan_ubsan(tmp_path):
    cc = shutil.which("gcc")
    if cc is None or shutil.which("make") is None:
        pytest.skip("no gcc/make")
    csrc = os.path.join(ROOT, "dgl-1_amd", "csrc")
    subprocess.check_call(["make", "-s", "-j8", "-C", csrc, "asan"])
    libdir = os.path.join(ROOT, "dgl-1_amd", "build_asan")
    exe = str(tmp_path / "weighted_sample_sanitize")
    subprocess.check_call([
        cc, "-std=c99", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
        "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "c_client", "weighted_sample_sanitize.c"),
        "-o", exe, "-L", libdir, "-ldgl_hip_asan", "-lm", "-Wl,-rpath," + libdir])
    supp = tmp_path / "lsan.supp"
    # leaks inside the ROCm runtime's own one-time initialisation are not ours
    supp.write_text("leak:libamdhip64\nleak:libhsa-runtime64\nleak:librocprofiler\n")
    env = dict(os.environ,
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               LSAN_OPTIONS="suppressions=%s" % supp,
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
    assert "weighted_sample_sanitize ok" in res.stdout
