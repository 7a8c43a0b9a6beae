"""CPU: the host half of the device JPEG decoder through the C ABI -- ntk_jpeg_parse (marker walk, descriptor, unstuffing),
ntk_jpeg_decode_workspace_bytes, and the refusals of ntk_jpeg_decode_batch, which fire on the host before anything is launched (no
GPU is needed), naming the offending value in ntk_last_error.  Every file of the synthetic corpus (tests/jpeg_write.py: table
indices 2 and 3, fill bytes, repeated DRI / DHT / DQT, ...) is accepted, and its descriptor, unstuffed stream and segment offsets
are those of the Python restatement.  A scan without EOI is accepted as well: the documented difference to Pillow."""
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as J  # noqa: E402
import jpeg_write as JW  # noqa: E402

ONE = ctypes.c_void_p(64)                       # non-null, aligned, never dereferenced: the checks fire first
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")
NAMES = ("ntk_jpeg_parse", "ntk_jpeg_decode_workspace_bytes", "ntk_jpeg_decode_batch")


@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


@pytest.mark.parametrize("name,nargs", zip(NAMES, (9, 4, 13)))
def test_symbols_are_declared_exported_and_bound(L, name, nargs):
    from ntmtrack import _lib
    assert re.search(r"^int %s\(" % name, open(HEADER).read(), re.M), "%s is not declared in include/ntmtrack.h" % name
    assert hasattr(L, name), "libntmtrack_hip.so does not export %s" % name
    assert name in _lib.exported_symbols()
    fn = getattr(L, name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs


def test_the_descriptor_constants_of_the_header_are_the_ones_python_uses():
    from ntmtrack import data
    d = {k: int(v) for k, v in re.findall(r"#define (NTK_JPEG_\w+)\s+(-?\d+)", open(HEADER).read())}
    assert d["NTK_JPEG_DESC_BYTES"] == data.JPEG_DESC_BYTES == 7936
    assert d["NTK_JPEG_DESC_HDR_WORDS"] == data.JPEG_DESC_HDR_WORDS
    assert d["NTK_JPEG_HOST_PATH"] == data.JPEG_HOST_PATH and d["NTK_JPEG_HOST_PATH"] > 0
    assert d["NTK_JPEG_MIN_SIDE"] == data.JPEG_MIN_SIDE == 16
    assert d["NTK_JPEG_WS_BYTES_PER_BLOCK"] == data.JPEG_WS_BYTES_PER_BLOCK
    words = {k[len("NTK_JPEG_DESC_"):]: v for k, v in d.items() if k.startswith("NTK_JPEG_DESC_") and k not in
             ("NTK_JPEG_DESC_BYTES", "NTK_JPEG_DESC_HDR_WORDS")}
    assert words == data.JPEG_DESC
    status = {v: k for k, v in d.items() if k.startswith("NTK_JPEG_STATUS_")}
    assert sorted(status) == sorted(data.JPEG_STATUS)


@pytest.mark.parametrize("size,sub,kw,want", [
    ((48, 64), 0, {}, ((1, 1), 0, 1)),
    ((33, 47), 1, {}, ((2, 1), 0, 1)),
    ((33, 47), 2, {"restart_marker_blocks": 2}, ((2, 2), 2, 5)),          # 3 x 3 MCUs of 16 x 16 -> ceil(9 / 2)
    ((40, 72), 1, {"restart_marker_rows": 1}, ((2, 1), 5, 5)),            # 5 MCUs a row, 5 rows
    ((17, 23), 0, {"restart_marker_blocks": 2}, ((1, 1), 2, 5)),          # 3 x 3 MCUs of 8 x 8
])
def test_pillow_files_report_size_sampling_restart_and_segments(size, sub, kw, want):
    from ntmtrack import data
    p = data.parse_jpeg(J.encode(J.image(size[0], size[1], "noise"), quality=90, subsampling=sub, **kw))
    assert (p.height, p.width, p.components) == (size[0], size[1], 3)
    assert (p.sampling, p.restart_interval, p.n_segments) == want
    assert p.segments[0] == 0 and p.segments[-1] == p.stream_bytes == p.stream.size and np.all(np.diff(p.segments) > 0)


def test_a_gray_file_has_one_component_and_one_block_per_mcu(tmp_path):
    from ntmtrack import data
    path = tmp_path / "gray.jpg"
    path.write_bytes(J.encode(J.image(40, 72, "smooth")[:, :, 0].copy(), quality=90))
    p = data.parse_jpeg(str(path))
    assert (p.height, p.width, p.components, p.sampling, p.mcus) == (40, 72, 1, (1, 1), (5, 9))


def test_unstuffed_bytes_equal_a_python_restatement():
    from ntmtrack import data
    data_ = J.encode(J.image(48, 64, "noise"), quality=100, subsampling=0, restart_marker_blocks=2)
    info = J.parse(data_)
    assert b"\xff\x00" in data_[info["scan_start"]:], "the fixture must contain stuffed bytes"
    dst = np.full(len(data_), 0xAB, np.uint8)
    p = data.parse_jpeg(data_, dst=dst)
    assert p.stream.tobytes() == info["stream"] and list(p.segments) == info["segments"]
    assert np.all(dst[p.stream_bytes:] == 0xAB), "bytes behind the stream were written"


def _progressive():
    return J.encode(J.image(32, 32, "smooth"), quality=90, progressive=True)


def _png():
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(J.image(32, 32, "smooth")).save(buf, "PNG")
    return buf.getvalue()


def _cmyk():
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(J.image(32, 32, "smooth")).convert("CMYK").save(buf, "JPEG")
    return buf.getvalue()


def _base():
    return bytearray(J.encode(J.image(32, 32, "smooth"), quality=90, subsampling=0))


def _too_many_short_codes():
    """The standard DC table (0, 1, 5, 1, ... codes of length 1, 2, 3, ...) with three codes of length 1 and as many fewer of length
    3: the same number of values, but length 1 has room for two codes."""
    b = _base()
    at = bytes(b).index(b"\xff\xc4") + 5
    assert list(b[at:at + 3]) == [0, 1, 5]
    b[at], b[at + 2] = 3, 2
    return bytes(b)


def _patched(marker, offset, value, insert=None):
    """The baseline 4:4:4 file with byte `offset` of the first `marker` segment's body set to `value` (or `insert` put before
    that segment)."""
    b = _base()
    at = bytes(b).index(bytes([0xFF, marker]))
    if insert is not None:
        return bytes(b[:at] + insert + b[at:])
    b[at + 4 + offset] = value
    return bytes(b)


HOST_PATH_CASES = {
    "not a jpeg": _png,
    "progressive": _progressive,
    "four components": _cmyk,
    "extended sequential (SOF1)": lambda: bytes(_base()).replace(b"\xff\xc0", b"\xff\xc1", 1),
    "lossless (SOF3)": lambda: bytes(_base()).replace(b"\xff\xc0", b"\xff\xc3", 1),
    "arithmetic (SOF9)": lambda: bytes(_base()).replace(b"\xff\xc0", b"\xff\xc9", 1),
    "12-bit samples": lambda: _patched(0xC0, 0, 12),
    "16-bit quantisation table": lambda: _patched(0xDB, 0, 0x10),
    "scan without all components": lambda: _patched(0xDA, 0, 0, insert=b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"),
    "DNL marker": lambda: _patched(0xDA, 0, 0, insert=b"\xff\xdc\x00\x04\x00\x20"),
    "luma sampled 1x2": lambda: _patched(0xC0, 7, 0x12),
    "chroma sampled 2x1": lambda: _patched(0xC0, 10, 0x21),
    "Adobe marker without JFIF": lambda: bytes(_base()).replace(b"\xff\xe0\x00\x10JFIF\x00", b"\xff\xee\x00\x10Adobe", 1),
    "component ids R G B without JFIF": lambda: _patched(0xC0, 6, ord("R")).replace(b"JFIF", b"JFXX", 1),
    "a side below 16": lambda: J.encode(J.image(15, 40, "smooth"), quality=90),
    "a second scan": lambda: bytes(_base())[:-2] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00\x00\xff\xd9",
}


@pytest.mark.parametrize("case", sorted(HOST_PATH_CASES))
def test_files_that_are_not_for_the_device_get_the_host_path_code(L, case):
    from ntmtrack import data
    raw = HOST_PATH_CASES[case]()
    desc = np.full(data.JPEG_DESC_BYTES, 0xFF, np.uint8)
    rc, _s, _n = data._jpeg_parse_raw(raw, desc, None, 0, 0, None, 0, 0, case)
    assert rc == data.JPEG_HOST_PATH, case
    assert desc[:128].view(np.int32)[data.JPEG_DESC["NCOMP"]] == 0, "a host-path descriptor must tell the device to skip the frame"
    assert data.parse_jpeg(raw) is None


def test_the_unpatched_base_file_is_accepted():
    from ntmtrack import data
    assert data.parse_jpeg(bytes(_base())) is not None
    assert data.parse_jpeg(bytes(_base()).replace(b"\xff\xe0\x00\x10JFIF", b"\xff\xe1\x00\x10Exif", 1)) is not None   # ids 1, 2, 3


@pytest.mark.parametrize("case,raw,named", [
    ("segment length past the end", lambda: _patched(0xDB, -2, 0xFF), b"length"),
    ("segment length below 2", lambda: bytes(_base()).replace(b"\xff\xdb\x00\x43", b"\xff\xdb\x00\x01", 1), b"length 1"),
    ("quantisation table index 5", lambda: _patched(0xDB, 0, 0x05), b"index 5"),
    ("Huffman table index 4", lambda: _patched(0xC4, 0, 0x04), b"index 4"),
    ("more Huffman codes than fit", _too_many_short_codes, b"more codes"),
    ("more Huffman values than the segment has", lambda: _patched(0xC4, 16, 200), b"values in"),
    ("file ends inside a segment", lambda: bytes(_base())[:30], b"leaves the file"),
])
def test_malformed_files_get_an_error_and_a_message(L, case, raw, named):
    from ntmtrack import _lib, data
    with pytest.raises(_lib.NtkError) as e:
        data.parse_jpeg(raw())
    assert named.decode() in str(e.value) and "(-5)" in str(e.value), str(e.value)
    assert named in L.ntk_last_error()


def test_a_file_cut_at_every_byte_position_never_crashes():
    """Every prefix of a small file with restart markers, in a buffer of exactly that length: an error, the host-path code, or --
    once the scan has begun -- an accepted file whose stream is a prefix of the whole file's."""
    from ntmtrack import _lib, data
    raw = J.encode(J.image(17, 23, "noise"), quality=50, subsampling=2, restart_marker_blocks=2)
    whole = data.parse_jpeg(raw)
    outcomes = {"error": 0, "host": 0, "accepted": 0}
    for cut in range(len(raw)):
        try:
            p = data.parse_jpeg(bytes(raw[:cut]))
        except _lib.NtkError:
            outcomes["error"] += 1
            continue
        if p is None:
            outcomes["host"] += 1
        else:
            outcomes["accepted"] += 1
            assert cut > J.parse(raw)["scan_start"] - 1
            assert whole.stream.tobytes().startswith(p.stream.tobytes()) and p.n_segments <= whole.n_segments
    assert outcomes["error"] > 100 and outcomes["host"] >= 4 and outcomes["accepted"] > 20, outcomes


def test_workspace_query_sizes_the_window_and_writes_the_offsets(L):
    from ntmtrack import data
    files = [J.encode(J.image(120, 200, "smooth"), quality=90, subsampling=2), J.encode(J.image(48, 64, "smooth"), quality=90, subsampling=0),
             _png()]
    probed = [data._probe_frame(f, "f%d" % i) for i, f in enumerate(files)]
    # 4:2:0, MCUs of 16 x 16: rows 17..40 -> chroma rows 7..21 -> MCU rows 0..2; columns 100..101 -> chroma 49..51 -> MCU columns 6..6
    packed = data.pack_jpeg_frames(probed, [(17, 100, 24, 2), (8, 8, 8, 8), (0, 0, 32, 32)], staging=data.Staging(pin=False))
    hdr = packed.staging.descs.numpy()[:3, :128].view(np.int32)
    offs = hdr[:, data.JPEG_DESC["WS_OFF"]:data.JPEG_DESC["WS_OFF"] + 2].copy().view(np.int64)[:, 0]
    assert list(offs) == [0, 3 * 1 * 6 * 192, 3 * 1 * 6 * 192 + 3 * 192]
    assert packed.jpeg.workspace_bytes == offs[2] + 192 and packed.jpeg.on_device == [True, True, False]
    table = packed.table.numpy().copy()
    table[0, 5] = 200                                                       # a rectangle that leaves the frame
    ws = ctypes.c_longlong(0)
    assert L.ntk_jpeg_decode_workspace_bytes(data._np_ptr(packed.staging.descs.numpy()), data._np_ptr(table), 3, ctypes.byref(ws)) == -1
    assert b"row 0" in L.ntk_last_error() and b"h=200" in L.ntk_last_error()
    assert L.ntk_jpeg_decode_workspace_bytes(None, data._np_ptr(table), 3, ctypes.byref(ws)) == -2
    assert L.ntk_jpeg_decode_workspace_bytes(data._np_ptr(packed.staging.descs.numpy()), data._np_ptr(table), 0, ctypes.byref(ws)) == -1
    assert b"n=0" in L.ntk_last_error()


def call(L, streams=ONE, streams_bytes=4096, descs=ONE, segments=ONE, n_segments=8, table=ONE, pixels=ONE, pixels_bytes=4096,
         workspace=ONE, workspace_bytes=1 << 20, status=ONE, n=2):
    return L.ntk_jpeg_decode_batch(streams, streams_bytes, descs, segments, n_segments, table, pixels, pixels_bytes, workspace,
                                   workspace_bytes, status, n, None)


@pytest.mark.parametrize("arg", ["streams", "descs", "segments", "table", "pixels", "workspace", "status"])
def test_decode_refuses_null_pointers(L, arg):
    assert call(L, **{arg: None}) == -2
    assert b"null" in L.ntk_last_error()


@pytest.mark.parametrize("kw,named", [
    ({"n": 0}, b"n=0"), ({"n": -1}, b"n=-1"), ({"n": 65536}, b"n=65536"),
    ({"streams_bytes": 0}, b"streams_bytes=0"), ({"n_segments": 0}, b"n_segments=0"), ({"pixels_bytes": -7}, b"pixels_bytes=-7"),
    ({"workspace_bytes": 383}, b"workspace_bytes=383 is short of 384"), ({"workspace_bytes": -1}, b"workspace_bytes=-1"),
])
def test_decode_refuses_bad_sizes_and_a_short_workspace_and_names_the_value(L, kw, named):
    assert call(L, **kw) == -1
    assert named in L.ntk_last_error()


# ------------------------------------------------------------------------------------------------------------------------------
# the synthetic corpus (tests/jpeg_write.py)
# ------------------------------------------------------------------------------------------------------------------------------

HUFF_BYTES = 512 + 72 + 72 + 256                # NtkJpegHuff: look uint16 [256], maxcode int32 [18], valoff int32 [18], val uint8 [256]


def _assert_descriptor_is_the_restatements(p, info):
    from ntmtrack import data
    nc = len(info["comps"])
    hs, vs = (info["comps"][0][1], info["comps"][0][2]) if nc == 3 else (1, 1)
    assert (p.height, p.width, p.components, p.sampling) == (info["H"], info["W"], nc, (hs, vs))
    assert p.mcus == (-(-info["H"] // (8 * vs)), -(-info["W"] // (8 * hs)))
    assert (p.restart_interval, p.n_segments) == (info["restart"], len(info["segments"]) - 1)
    D = data.JPEG_DESC
    for c in range(nc):
        assert (int(p.hdr[D["TQ"] + c]), int(p.hdr[D["TD"] + c]), int(p.hdr[D["TA"] + c])) == (info["comps"][c][3],) + info["scan"][c]
    quant = p.desc[128:128 + 512].view(np.uint16).reshape(4, 64)
    for t, q in info["quant"].items():
        assert np.array_equal(quant[t], q), "quantisation table %d" % t
    for (cls, t), (counts, vals) in info["huff"].items():
        h = p.desc[640 + (cls * 4 + t) * HUFF_BYTES:640 + (cls * 4 + t + 1) * HUFF_BYTES]
        maxcode, val = h[512:584].view(np.int32), h[656:]
        assert list(val[:len(vals)]) == list(vals), "Huffman table %d/%d: values" % (cls, t)
        code, want = 0, [-1] * 18
        for l in range(1, 17):
            if counts[l - 1]:
                want[l] = code + counts[l - 1] - 1
            code = (code + counts[l - 1]) << 1
        assert list(maxcode) == want, "Huffman table %d/%d: largest code per length" % (cls, t)
    assert p.stream.tobytes() == info["stream"] and list(p.segments) == info["segments"]
    assert p.stream_bytes == len(info["stream"])


@pytest.mark.parametrize("name", [n for n, _kw in JW.recipes()])
def test_every_corpus_file_is_accepted_and_its_descriptor_is_the_restatements(L, name):
    from ntmtrack import data
    raw = dict(JW.corpus())[name]
    desc = np.zeros(data.JPEG_DESC_BYTES, np.uint8)
    rc, _s, _n = data._jpeg_parse_raw(raw, desc, None, 0, 0, None, 0, 0, name)
    assert rc == 0, "%s: ntk_jpeg_parse returned %d" % (name, rc)
    dst = np.full(len(raw), 0xAB, np.uint8)
    p = data.parse_jpeg(raw, dst=dst)
    _assert_descriptor_is_the_restatements(p, J.parse(raw))
    assert np.all(dst[p.stream_bytes:] == 0xAB), "bytes behind the stream were written"


def test_a_scan_without_eoi_is_accepted_where_pillow_raises():
    """include/ntmtrack.h documents the difference: decode="host" raises on such a file, decode="device" decodes what the scan
    holds (all of the image here; a scan that ends early is NTK_JPEG_STATUS_TRUNCATED)."""
    from ntmtrack import data
    whole = dict(JW.corpus())["s444_noise3_33x47"]
    assert whole.endswith(b"\xff\xd9")
    cut = whole[:-2]
    with pytest.raises(OSError):
        J.pillow_decode(cut)
    p, q = data.parse_jpeg(cut), data.parse_jpeg(whole)
    assert p is not None and p.stream.tobytes() == q.stream.tobytes() and list(p.segments) == list(q.segments)
    assert np.array_equal(p.desc, q.desc)
