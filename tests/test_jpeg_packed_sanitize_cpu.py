"""The packed entry point of the host JPEG decoder under the address and undefined-behaviour sanitizers, on the CPU:
fastvim_amd/csrc/jpeg_host.cpp is compiled together with tools/jpeg_packed_check.cpp -- a program with its own ``main`` -- by
the host compiler with ``-fsanitize=address,undefined``, and that program runs ``fv_jpeg_entropy_decode_packed`` on every
fixture, on every truncation of one small fixture and on 4000 seeded byte mutations, each once into a heap buffer of
exactly ``fv_jpeg_packed_bound`` bytes and once into one of a third of that.  It must exit clean.  Nothing is loaded into
Python and nothing is preloaded; skipped where the compiler cannot link the sanitizer runtime."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_host_decoder_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link or run the sanitizer runtime")
    exe = tmp_path / "jpeg_packed_check"
    r = subprocess.run([cxx, *flags, "-o", str(exe), os.path.join(ROOT, "tools", "jpeg_packed_check.cpp"),
                        os.path.join(ROOT, "fastvim_amd", "csrc", "jpeg_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
    names = [str(n) for n in z["names"]]
    names.sort(key=lambda n: (n != "17x23_420_q75_noise", n))          # the first file is the one truncated everywhere
    files = []
    for n in names:
        p = tmp_path / (n + ".jpg")
        p.write_bytes(z["jpg_" + n].tobytes())
        files.append(str(p))
    r = subprocess.run([str(exe), *files], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert f"files {len(names)} served {len(names) - 1} bad 0;" in r.stdout, r.stdout
