"""CPU: the device JPEG decoder's host-callable parts (csrc/jpeg_parse.h: marker walk and unstuffing; csrc/jpeg_entropy.h: the
per-segment Huffman loop the GPU runs and the MCU window) in a stand-alone program built with the address and
undefined-behaviour sanitizers (tests/host/jpeg_decode_check.cpp): the whole fixture grid decodes to the coefficients of the NumPy
restatement (tests/jpeg_util.py), and thousands of seeded corruptions -- bytes flipped in headers and scans, truncations, restart
intervals that disagree with the data, headers cut at every byte -- end in a status, a refusal or the host path, never in an
access outside a buffer.  The bounds of the entropy loop are proven here, on the CPU, before a GPU sees a malformed stream.  The
truncated file of tests/test_jpeg_decode_gpu.py is among the files checked.

The same holds for the synthetic corpus of tests/jpeg_write.py, whose files reach what Pillow's encoder never writes (table indices 2
and 3, chain and single-code Huffman tables, DC differences of category 11, ZRL rows, blocks without an EOB, fill bytes, repeated
DRI / DHT / DQT, more than 128 restart segments): each file is one on which the restatement equals Pillow -- the condition for
being in the corpus --, the corpus covers every value it was built for with every sampling, and the sanitizer program decodes
every file of it clean, to the restatement's coefficients, before tests/test_jpeg_synthetic_gpu.py sends it to a device."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as J  # noqa: E402
import jpeg_write as JW  # noqa: E402

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


# ------------------------------------------------------------------------------------------------------------------------------
# the synthetic corpus (tests/jpeg_write.py)
# ------------------------------------------------------------------------------------------------------------------------------

RECIPES = ("dcwalk", "acends", "runs", "ones", "onesfill", "dc0q255", "noise3", "smooth3", "manyseg")
CORPUS_NAMES = [name for name, _kw in JW.recipes()]


@pytest.fixture(scope="module")
def corpus():
    return dict(JW.corpus())


def _by_sampling(sampling):
    return [(name, kw) for name, kw in JW.recipes() if kw["sampling"] == sampling]


def test_the_corpus_is_a_fixed_list_with_every_recipe_in_every_sampling(corpus):
    assert len(CORPUS_NAMES) == len(set(CORPUS_NAMES)) == len(corpus) == len(RECIPES) * len(JW.SAMPLINGS) == 36
    assert [n for n, _d in JW.corpus()] == CORPUS_NAMES
    for sampling in JW.SAMPLINGS:
        assert [n.split("_")[1] for n, _kw in _by_sampling(sampling)] == list(RECIPES)
    assert JW.corpus() == JW.corpus() and dict(JW.corpus()) == {n: JW.write(**kw) for n, kw in JW.recipes()}, "the corpus is seeded"
    for name, data in corpus.items():
        info = J.parse(data)
        assert min(info["H"], info["W"]) >= 16 and (name.split("_")[1] == "manyseg" or max(info["H"], info["W"]) <= 80), name


def test_the_standard_tables_of_the_writer_are_the_ones_pillow_writes():
    info = J.parse(J.encode(J.image(32, 32, "noise"), quality=90, subsampling=2))
    std = {(0, 0): JW.STD_DC_LUMA, (1, 0): JW.STD_AC_LUMA, (0, 1): JW.STD_DC_CHROMA, (1, 1): JW.STD_AC_CHROMA}
    assert {k: (list(c), list(v)) for k, (c, v) in info["huff"].items()} == {k: (list(c), list(v)) for k, (c, v) in std.items()}


@pytest.mark.parametrize("name", CORPUS_NAMES)
def test_the_restatement_is_pillow_on_every_corpus_file(corpus, name):
    """The condition for being in the corpus.  A generator whose file fails it leaves the contract's domain (libjpeg-turbo's SIMD
    inverse DCT saturates 16-bit intermediates): its parameters change, never this assertion."""
    want = J.pillow_decode(corpus[name])
    got = J.decode(corpus[name])
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (name, np.count_nonzero(got != want))


@pytest.mark.parametrize("name", CORPUS_NAMES)
def test_the_writer_round_trips_through_the_restatement(corpus, name):
    """What the writer was given is what the file says: coefficients, tables, table choices, sizes and the restart interval."""
    kw = dict(JW.recipes())[name]
    info = J.parse(corpus[name])
    coef, hs, vs = J.coefficients(info)
    assert np.array_equal(coef, kw["coef"]) and (len(info["comps"]), hs, vs) == JW.SAMPLINGS[kw["sampling"]]
    assert (info["H"], info["W"], info["restart"]) == (kw["H"], kw["W"], kw["restart"])
    assert [c[3] for c in info["comps"]] == list(kw["comp_quant"]) and info["scan"] == list(kw["comp_huff"])
    assert all(np.array_equal(info["quant"][t], q) for t, q in kw["quant"].items()) and set(info["quant"]) == set(kw["quant"])
    assert {k: (list(c), list(v)) for k, (c, v) in info["huff"].items()} == {k: (list(c), list(v)) for k, (c, v) in kw["huff"].items()}
    total = coef.shape[0] * coef.shape[1]
    assert len(info["segments"]) - 1 == (-(-total // kw["restart"]) if kw["restart"] else 1)


@pytest.mark.parametrize("sampling", sorted(JW.SAMPLINGS))
def test_the_corpus_reaches_the_entropy_extremes_with_every_sampling(corpus, sampling):
    st = [JW.stats(kw["coef"], sampling, kw["restart"]) for _n, kw in _by_sampling(sampling)]
    union = lambda key: set().union(*[s[key] for s in st])
    ends = {0} | {sg * v for s in range(1, 12) for v in (1 << (s - 1), (1 << s) - 1) for sg in (1, -1)}
    assert ends <= union("dc_diff"), "DC differences never met: %s" % sorted(ends - union("dc_diff"))
    assert set(JW.AC_ENDS) <= union("ac_value"), "AC values never met: %s" % sorted(set(JW.AC_ENDS) - union("ac_value"))
    assert {r for r, _s in union("run_size")} == set(range(16)) and {s for _r, s in union("run_size")} == set(range(1, 11))
    assert union("zrl_rows") == {1, 2, 3}
    assert all(sum(s[key] for s in st) > 0 for key in ("no_eob", "zero_blocks", "dc_only"))
    ones = dict(_by_sampling(sampling))["%s_ones_17x23" % sampling]
    scan = corpus["%s_ones_17x23" % sampling]
    scan = scan[J.parse(scan)["scan_start"]:]
    total = ones["coef"].shape[0] * ones["coef"].shape[1]
    assert ones["restart"] == 1 and sum(scan.count(bytes([0xFF, 0x00, 0xFF, 0xD0 + k])) for k in range(8)) == total - 1, \
        "every segment of the all-ones file must end in a stuffed FF right before its restart marker"
    assert scan.count(b"\xff\x00") * 8 > len(scan), "the all-ones file is meant to be dense with FF 00"


def _lengths(table):
    return {l for l, n in enumerate(table[0], 1) if n}


@pytest.mark.parametrize("sampling", sorted(JW.SAMPLINGS))
def test_the_corpus_carries_every_table_restart_and_layout_value_with_every_sampling(corpus, sampling):
    """The axes of the corpus, read back from the files' own bytes where the bytes show them.  (Three tables for three components
    need three components: those two values are met with every colour sampling.)"""
    files = {n.split("_")[1]: (kw, corpus[n], J.parse(corpus[n])) for n, kw in _by_sampling(sampling)}
    colour = sampling != "gray"
    kw, data, info = files["acends"]
    # Huffman: chain tables -- one code per length, the longest 16 bits, most of them beyond the 8-bit lookup
    chains = [t for t in info["huff"].values() if max(t[0]) == 1 and len(t[1]) > 1]
    assert chains and all(max(_lengths(t)) == 16 for t in chains) and any(len(_lengths(t) & set(range(9, 17))) == 8 for t in info["huff"].values())
    assert {t for _c, t in info["huff"]} == {2, 3}                                                     # Huffman tables 2 and 3
    assert set(info["quant"]) == {2, 3} and [c[3] for c in info["comps"]][0] == 3                       # quantisation tables 2 and 3
    assert info["restart"] == kw["coef"].shape[0] * kw["coef"].shape[1]                                 # interval = the MCU count
    head = data[:info["scan_start"]]
    assert head.count(b"\xff\xdd") == 2 and head.count(b"\xff\xff\xdb") == 2 and head.count(b"\xff\xff\xc4") == 2    # DRI twice; decoy + merged
    assert head.count(b"\xff\xff\xfe") == 2 and b"\xff\xff\xe1" in head and b"JFIF" in head               # COM, APP1, fill bytes
    assert data.endswith(b"\xff\xff\xd9") and [c[0] for c in info["comps"]] == [0, 1, 2][:len(info["comps"])]
    # a single-code DC table; 255 in the quantisation table under coefficients of at most 3; an interval beyond the MCU count
    kw, data, info = files["dc0q255"]
    assert info["huff"][(0, 2)] == ([1] + [0] * 15, [0]) and int(info["quant"][1].max()) == 255 and np.abs(kw["coef"]).max() <= 3
    assert info["restart"] > kw["coef"].shape[0] * kw["coef"].shape[1] and data[:info["scan_start"]].count(b"\xff\xdd") == 2
    # one table pair shared by all components; quantisation all ones
    kw, data, info = files["dcwalk"]
    assert set(info["huff"]) == {(0, 0), (1, 0)} and set(info["scan"]) == {(0, 0)} and all(np.all(q == 1) for q in info["quant"].values())
    # three tables for three components (Huffman and quantisation), a redefined DHT and DQT, zero padding
    kw, data, info = files["noise3"]
    if colour:
        assert len(set(info["scan"])) == 3 and len({td for td, _ta in info["scan"]}) == 3 and len({ta for _td, ta in info["scan"]}) == 3
        assert len({c[3] for c in info["comps"]}) == 3 and len({q.tobytes() for q in info["quant"].values()}) == 3
        assert len({(tuple(info["huff"][(1, ta)][0]), tuple(info["huff"][(1, ta)][1])) for _td, ta in info["scan"]}) == 3
    head = data[:info["scan_start"]]
    assert head.count(b"\xff\xc4") == 2 and head.count(b"\xff\xdb") == 2 and kw["decoy_dht"] and kw["decoy_dqt"] and not kw["pad_ones"]
    # skewed frequency tables: the 16-bit limit was at work; an interval that divides neither a row nor the frame; no JFIF segment
    kw, data, info = files["runs"]
    total, row = kw["coef"].shape[0] * kw["coef"].shape[1], kw["coef"].shape[1]
    assert info["restart"] == 7 and total % 7 and row % 7 and b"JFIF" not in data and [c[0] for c in info["comps"]] == [1, 2, 3][:len(info["comps"])]
    assert any(max(_lengths(t)) == 16 and max(t[0]) > 1 for t in info["huff"].values())
    assert sum(data.count(bytes([0xFF, 0xFF, 0xD0 + k])) for k in range(8)) >= len(info["segments"]) - 2  # fill bytes before RSTn
    # interval 1, with and without fill bytes; separate and merged table segments
    assert files["ones"][2]["restart"] == files["onesfill"][2]["restart"] == 1
    assert files["ones"][1][:files["ones"][2]["scan_start"]].count(b"\xff\xc4") == len(files["ones"][2]["huff"])
    assert files["onesfill"][1][:files["onesfill"][2]["scan_start"]].count(b"\xff\xc4") == 1
    # more than 128 segments
    assert len(files["manyseg"][2]["segments"]) - 1 > 128
    if sampling == "gray":
        assert len(files["manyseg"][2]["segments"]) - 1 == 250


@pytest.mark.parametrize("sampling", sorted(JW.SAMPLINGS))
def test_the_corpus_has_pixels_that_clamp_at_both_ends_after_the_idct_and_after_the_colour_conversion(corpus, sampling):
    counts = np.array([[J.clamp_counts(corpus[n])] for n, _kw in _by_sampling(sampling)]).reshape(-1, 4).sum(axis=0)
    print("%s: samples the inverse DCT clamps at 0 / 255: %d / %d; colour values clamped at 0 / 255: %d / %d" % ((sampling,) + tuple(counts)))
    assert counts[0] > 0 and counts[1] > 0
    assert sampling == "gray" or (counts[2] > 0 and counts[3] > 0)


def test_segment_decoder_under_sanitizers_on_the_synthetic_corpus(exe, tmp_path):
    files = JW.corpus()
    for name, data in files:
        (tmp_path / name).write_bytes(data)
    (tmp_path / "files.txt").write_text("".join(name + "\n" for name, _d in files))
    run = subprocess.run([exe, str(tmp_path), str(CORRUPTIONS_PER_FILE * 4)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True)
    assert run.returncode == 0 and "jpeg decode check: ok" in run.stdout, run.stdout[-4000:]
    assert "good files: %d decodes" % (9 * len(files)) in run.stdout, run.stdout[-4000:]      # whole + 8 rectangles, all clean
    for name, data in files:
        want, _hs, _vs = J.coefficients(J.parse(data))
        got = np.fromfile(str(tmp_path / (name + ".coef")), dtype=np.int16)
        assert got.size == want.size and np.array_equal(got.astype(np.int64), want.reshape(-1)), "%s: coefficients differ" % name


def test_a_scan_without_eoi_is_pillows_error_and_the_device_decoders_image(exe, tmp_path):
    """The documented difference (include/ntmtrack.h): Pillow refuses a file that ends without EOI, the device path decodes what
    the scan holds -- here all of it, clean, to the coefficients of the whole file."""
    whole = dict(JW.corpus())["s420_runs_33x47"]
    assert whole.endswith(b"\xff\xff\xd9")
    cut = whole[:-3]
    with pytest.raises(OSError):
        J.pillow_decode(cut)
    (tmp_path / "cut.jpg").write_bytes(cut)
    (tmp_path / "files.txt").write_text("cut.jpg\n")
    run = subprocess.run([exe, str(tmp_path), "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0 and "jpeg decode check: ok" in run.stdout, run.stdout[-4000:]
    want, _hs, _vs = J.coefficients(J.parse(whole))
    assert np.array_equal(np.fromfile(str(tmp_path / "cut.jpg.coef"), dtype=np.int16).astype(np.int64), want.reshape(-1))
