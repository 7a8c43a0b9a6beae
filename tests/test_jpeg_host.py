"""CPU: the device JPEG decoder's host-callable parts (csrc/jpeg_parse.h: marker walk and unstuffing; csrc/jpeg_entropy.h: the
per-segment Huffman loop the GPU runs and the MCU window) in a stand-alone program built with the address and
undefined-behaviour sanitizers (tests/host/jpeg_decode_check.cpp): the whole fixture grid decodes to the coefficients of the NumPy
restatement (tests/jpeg_util.py), and thousands of seeded corruptions -- bytes flipped in headers and scans, truncations, restart
intervals that disagree with the data, headers cut at every byte -- end in a status, a refusal or the host path, never in an
access outside a buffer.  The bounds of the entropy loop are proven here, on the CPU, before a GPU sees a malformed stream.  The
truncated file of tests/test_jpeg_decode_gpu.py is among the files checked."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as J  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORRUPTIONS_PER_FILE = 15       # x 280 files = 4200


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise AssertionError("no C++ compiler found for the host check")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jpeg_host") / "jpeg_decode_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "ntm-tracker_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "jpeg_decode_check.cpp"), "-o", out])
    return out


def test_the_restatement_is_pillow_on_the_whole_grid():
    bad = [name for name, data in J.grid() if not np.array_equal(J.decode(data), J.pillow_decode(data))]
    assert not bad, "the NumPy restatement differs from Pillow on %d files: %s" % (len(bad), bad[:8])


def test_segment_decoder_under_sanitizers(exe, tmp_path):
    files = J.grid()
    for name, data in files:
        (tmp_path / name).write_bytes(data)
    (tmp_path / "files.txt").write_text("".join(name + "\n" for name, _d in files))
    run = subprocess.run([exe, str(tmp_path), str(CORRUPTIONS_PER_FILE)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True)
    assert run.returncode == 0 and "jpeg decode check: ok" in run.stdout, run.stdout[-4000:]
    for name, data in files:
        want, _hs, _vs = J.coefficients(J.parse(data))
        got = np.fromfile(str(tmp_path / (name + ".coef")), dtype=np.int16)
        assert got.size == want.size and np.array_equal(got.astype(np.int64), want.reshape(-1)), "%s: coefficients differ" % name


def test_the_truncated_file_of_the_gpu_test_is_flagged_on_the_host(exe, tmp_path):
    """The file tests/test_jpeg_decode_gpu.py cuts to 40 % of its scan: the parser accepts it and the segment decoder flags it
    (exit 1 of the check program's clean-decode requirement, with the status named), under the sanitizers, before the GPU test
    sends it to a device."""
    data = J.truncated_file()
    (tmp_path / "cut.jpg").write_bytes(data)
    (tmp_path / "files.txt").write_text("cut.jpg\n")
    run = subprocess.run([exe, str(tmp_path), "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 1 and "cut.jpg: expected a clean decode, got 102" in run.stdout, run.stdout[-4000:]
