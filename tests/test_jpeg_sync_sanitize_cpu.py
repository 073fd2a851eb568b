"""The index-free JPEG path under the address and undefined-behaviour sanitizers, on the CPU: tools/jpeg_sync_check.cpp -- a
program with its own ``main`` -- is compiled together with fastvim_amd/csrc/jpeg_host.cpp and the core headers
fastvim_amd/csrc/jpeg_sync_core.h and jpeg_huff_core.h (the text the device compiles) by the host compiler with
``-fsanitize=address,undefined``.  The program stages every fixture with S in {1, 3, 1000} and subsequences of 16, 64 and
128 bytes, whole images and inner windows, into heap blocks of exactly the staged size, runs ``fv_jpeg_sync_host`` and then
every ``fv_jpeg_huff`` lane through the core, compares with ``fv_jpeg_entropy_decode``, then runs 4000 seeded mutations of
the staged scan and 4000 of the sync job's words.  It must exit clean and terminate.  Nothing is loaded into Python and
nothing is preloaded; skipped where the compiler cannot link the sanitizer runtime."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sync_core_and_stage_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link or run the sanitizer runtime")
    exe = tmp_path / "jpeg_sync_check"
    r = subprocess.run([cxx, *flags, "-o", str(exe), os.path.join(ROOT, "tools", "jpeg_sync_check.cpp"),
                        os.path.join(ROOT, "fastvim_amd", "csrc", "jpeg_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files, indexable = [], 0
    for npz in ("jpeg_cases.npz", "jpeg_index_cases.npz"):
        z = np.load(os.path.join(ROOT, "tests", "golden", npz))
        for n in (str(n) for n in z["names"]):
            p = tmp_path / (n + ".jpg")
            p.write_bytes(z["jpg_" + n].tobytes())
            files.append(str(p))
            indexable += "_rst" not in n and "progressive" not in n
    r = subprocess.run([str(exe), *files], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert f"files {len(files)} staged {indexable} refused {len(files) - indexable} bad 0;" in r.stdout, r.stdout
