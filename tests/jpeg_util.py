"""A NumPy restatement of baseline JPEG decoding with libjpeg's default integer pipeline (Huffman decoding, dequantisation, the
13-bit "slow integer" inverse DCT, triangle chroma upsampling, YCbCr -> RGB), independent of the library's C code: the oracle for
the device decoder's intermediate results (coefficients, planes) and, against Pillow, the proof that the arithmetic stated in
include/ntmtrack.h is the one Pillow runs.  Also the Pillow-written fixture grid the JPEG tests share."""
import io
import itertools

import numpy as np

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                    47, 55, 62, 63])


def unstuff(scan):
    """Entropy-coded bytes of a scan (up to its first non-restart marker) -> (bytes without stuffing, segment offsets + end,
    length consumed)."""
    out, segs, p = bytearray(), [0], 0
    while p < len(scan):
        c = scan[p]
        if c != 0xFF:
            out.append(c); p += 1
        elif p + 1 >= len(scan):
            p = len(scan)
        elif scan[p + 1] == 0:
            out.append(0xFF); p += 2
        elif scan[p + 1] == 0xFF:
            p += 1
        elif 0xD0 <= scan[p + 1] <= 0xD7:
            segs.append(len(out)); p += 2
        else:
            break
    segs.append(len(out))
    return bytes(out), segs, p


def parse(data):
    """Markers of a baseline file -> dict(H, W, comps=[(id, h, v, tq)], quant {t: [64] natural}, huff {(class, t): (counts, vals)},
    restart, scan=[(td, ta)], stream, segments)."""
    assert data[:2] == b"\xff\xd8"
    p, info = 2, {"quant": {}, "huff": {}, "restart": 0}
    while True:
        assert data[p] == 0xFF
        while data[p + 1] == 0xFF:             # fill bytes before a marker
            p += 1
        m = data[p + 1]
        L = (data[p + 2] << 8) | data[p + 3]
        b = data[p + 4:p + 2 + L]
        p += 2 + L
        if m == 0xC0:
            info["H"], info["W"] = (b[1] << 8) | b[2], (b[3] << 8) | b[4]
            info["comps"] = [(b[6 + 3 * c], b[7 + 3 * c] >> 4, b[7 + 3 * c] & 15, b[8 + 3 * c]) for c in range(b[5])]
        elif m == 0xDB:
            i = 0
            while i < len(b):
                q = np.zeros(64, np.int64)
                q[NATURAL] = np.frombuffer(b[i + 1:i + 65], np.uint8)
                info["quant"][b[i] & 15] = q
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(b):
                counts = list(b[i + 1:i + 17])
                info["huff"][(b[i] >> 4, b[i] & 15)] = (counts, list(b[i + 17:i + 17 + sum(counts)]))
                i += 17 + sum(counts)
        elif m == 0xDD:
            info["restart"] = (b[0] << 8) | b[1]
        elif m == 0xDA:
            info["scan"] = [(b[2 + 2 * c] >> 4, b[2 + 2 * c] & 15) for c in range(b[0])]
            break
    info["scan_start"] = p
    info["stream"], info["segments"], _ = unstuff(data[p:])
    return info


def _codes(counts, vals):
    """(length, code) -> value"""
    table, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            table[(l, code)] = vals[k]
            code += 1; k += 1
        code <<= 1
    return table


class _Bits(object):
    def __init__(self, data):
        self.data, self.pos = data, 0          # pos in bits

    def bit(self):
        byte = self.data[self.pos >> 3] if (self.pos >> 3) < len(self.data) else 0
        v = (byte >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return v

    def take(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.bit()
            if (l, code) in table:
                return table[(l, code)]
        raise ValueError("no Huffman code matches")


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def coefficients(info):
    """-> (coef int64 [mcus_y, mcus_x, blocks_per_mcu, 64] natural order, hs, vs)"""
    comps = info["comps"]
    hs, vs = (comps[0][1], comps[0][2]) if len(comps) == 3 else (1, 1)
    H, W = info["H"], info["W"]
    mcus_x, mcus_y = -(-W // (8 * hs)), -(-H // (8 * vs))
    nluma = hs * vs
    bpm = nluma + 2 if len(comps) == 3 else 1
    tables = {k: _codes(*v) for k, v in info["huff"].items()}
    coef = np.zeros((mcus_y * mcus_x, bpm, 64), np.int64)
    total = mcus_x * mcus_y
    interval = info["restart"] or total
    segs = info["segments"]
    for k in range(len(segs) - 1):
        r = _Bits(info["stream"][segs[k]:segs[k + 1]])
        pred = [0, 0, 0]
        for mcu in range(k * interval, min((k + 1) * interval, total)):
            for b in range(bpm):
                c = 0 if b < nluma else b - nluma + 1
                td, ta = info["scan"][c]
                s = r.symbol(tables[(0, td)])
                pred[c] += _extend(r.take(s), s) if s else 0
                coef[mcu, b, 0] = pred[c]
                i = 1
                while i < 64:
                    sym = r.symbol(tables[(1, ta)])
                    run, size = sym >> 4, sym & 15
                    if size == 0:
                        if run != 15:
                            break
                        i += 16
                        continue
                    i += run
                    coef[mcu, b, NATURAL[i]] = _extend(r.take(size), size)
                    i += 1
    return coef.reshape(mcus_y, mcus_x, bpm, 64), hs, vs


def _idct8(v, shift):
    """v [..., 8] along the last axis, int64 (no value leaves int32's range on valid data)"""
    v0, v1, v2, v3, v4, v5, v6, v7 = [v[..., i] for i in range(8)]
    z1 = (v2 + v6) * 4433
    tmp2 = z1 - v6 * 15137
    tmp3 = z1 + v2 * 6270
    tmp0 = (v0 + v4) << 13
    tmp1 = (v0 - v4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = v7, v5, v3, v1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = 1 << (shift - 1)
    out = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return np.stack([(o + r) >> shift for o in out], axis=-1)


def idct_blocks(coef, quant, clip=True):
    """coef [..., 64] natural order, quant [64] -> uint8-range samples [..., 8, 8] (clip=False: before the range limit)"""
    v = (coef * quant).reshape(coef.shape[:-1] + (8, 8))
    v = np.swapaxes(_idct8(np.swapaxes(v, -1, -2), 11), -1, -2)        # columns
    v = _idct8(v, 18)                                                   # rows
    return np.clip(v + 128, 0, 255) if clip else v + 128


def planes(info, clip=True):
    """-> list of MCU-padded planes (int64), one per component"""
    coef, hs, vs = coefficients(info)
    my, mx, bpm, _ = coef.shape
    out = []
    nluma = hs * vs
    for c, comp in enumerate(info["comps"]):
        q = info["quant"][comp[3]]
        if c == 0:
            px = idct_blocks(coef[:, :, :nluma], q, clip).reshape(my, mx, vs, hs, 8, 8)
            out.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8))
        else:
            px = idct_blocks(coef[:, :, nluma + c - 1], q, clip)
            out.append(px.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
    return out, hs, vs


def upsample_h2v1(c, W):
    cn = (W + 1) // 2
    s = c[:, :cn]
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    even, odd = (3 * s + left + 1) >> 2, (3 * s + right + 2) >> 2
    even[:, 0], odd[:, -1] = s[:, 0], s[:, -1]
    return np.stack([even, odd], axis=-1).reshape(s.shape[0], 2 * cn)[:, :W]


def upsample_h2v2(c, H, W):
    cn_y, cn_x = (H + 1) // 2, (W + 1) // 2
    s = c[:cn_y, :cn_x]
    above = np.concatenate([s[:1], s[:-1]], axis=0)
    below = np.concatenate([s[1:], s[-1:]], axis=0)
    rows = np.stack([3 * s + above, 3 * s + below], axis=1).reshape(2 * cn_y, cn_x)[:H]
    v = rows
    left = np.concatenate([v[:, :1], v[:, :-1]], axis=1)
    right = np.concatenate([v[:, 1:], v[:, -1:]], axis=1)
    even, odd = (3 * v + left + 8) >> 4, (3 * v + right + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * v[:, 0] + 8) >> 4, (4 * v[:, -1] + 7) >> 4
    return np.stack([even, odd], axis=-1).reshape(H, 2 * cn_x)[:, :W]


def _rgb(info):
    """-> int64 [H, W, 3] before the last range limit (a gray file: Y three times, already within 0..255)"""
    H, W = info["H"], info["W"]
    pl, hs, vs = planes(info)
    Y = pl[0][:H, :W]
    if len(pl) == 1:
        return np.stack([Y, Y, Y], axis=-1)
    if hs == 1:
        cb, cr = pl[1][:H, :W], pl[2][:H, :W]
    elif vs == 1:
        cb, cr = upsample_h2v1(pl[1][:H], W), upsample_h2v1(pl[2][:H], W)
    else:
        cb, cr = upsample_h2v2(pl[1], H, W), upsample_h2v2(pl[2], H, W)
    cb, cr = cb - 128, cr - 128
    F = lambda x: int(x * 65536 + 0.5)
    R = Y + ((F(1.402) * cr + 32768) >> 16)
    G = Y + ((-F(0.34414) * cb - F(0.71414) * cr + 32768) >> 16)
    B = Y + ((F(1.772) * cb + 32768) >> 16)
    return np.stack([R, G, B], axis=-1)


def decode(data):
    """File bytes -> uint8 [H, W, 3], what np.asarray(Image.open(f).convert("RGB")) gives."""
    return np.clip(_rgb(parse(data)), 0, 255).astype(np.uint8)


def clamp_counts(data):
    """How often the two range limits of the pipeline act inside the image: -> ((samples the inverse DCT gives below 0, above
    255), (colour values below 0, above 255 after YCbCr -> RGB; (0, 0) for a gray file))."""
    info = parse(data)
    H, W = info["H"], info["W"]
    pl, hs, vs = planes(info, clip=False)
    lo = hi = 0
    for c, p in enumerate(pl):
        p = p[:H, :W] if c == 0 or hs == 1 else p[:-(-H // vs), :-(-W // hs)]
        lo, hi = lo + int(np.count_nonzero(p < 0)), hi + int(np.count_nonzero(p > 255))
    rgb = _rgb(info)
    return (lo, hi), (int(np.count_nonzero(rgb < 0)), int(np.count_nonzero(rgb > 255)))


# ------------------------------------------------------------------------------------------------------------------------------
# fixtures, written by Pillow at test time
# ------------------------------------------------------------------------------------------------------------------------------

def image(h, w, kind, seed=0):
    rng = np.random.default_rng(seed * 7919 + h * 131 + w)
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    ph = rng.uniform(0, 6.28, size=3)
    img = [127.5 + 120 * np.sin(ph[c] + x * (0.11 + 0.05 * c) + y * (0.07 + 0.03 * c)) for c in range(3)]
    return np.clip(np.stack(img, axis=-1), 0, 255).astype(np.uint8)


def encode(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr if arr.ndim == 3 else arr, "RGB" if arr.ndim == 3 else "L").save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


GRID_SIZES = ((16, 16), (17, 23), (33, 47), (40, 72), (48, 64))
RESTARTS = ({}, {"restart_marker_blocks": 2}, {"restart_marker_rows": 1})


def grid():
    """The device-decode grid: (name, file bytes) for sizes x noise/smooth x subsampling 0/1/2 (+ one gray) x quality 50/90/100 x
    restart off / blocks=2 / rows=1, plus optimize=True files."""
    files = []
    for (h, w), kind, sub, q, (ri, rs) in itertools.product(GRID_SIZES, ("noise", "smooth"), (0, 1, 2), (50, 90, 100),
                                                           enumerate(RESTARTS)):
        files.append(("%dx%d_%s_s%d_q%d_r%d" % (h, w, kind, sub, q, ri), encode(image(h, w, kind), quality=q, subsampling=sub, **rs)))
    for (h, w), rs in zip(GRID_SIZES, RESTARTS + RESTARTS):
        files.append(("%dx%d_gray" % (h, w), encode(image(h, w, "smooth")[:, :, 1].copy(), quality=90, **rs)))
    for (h, w), sub in zip(GRID_SIZES, (0, 1, 2, 2, 1)):
        files.append(("%dx%d_opt_s%d" % (h, w, sub), encode(image(h, w, "noise", 1), quality=92, subsampling=sub, optimize=True)))
    return files


def truncated_file():
    """A 40x72 4:2:0 noise file whose scan is cut to 40 % of its bytes (no restart markers, no EOI): the parser accepts it, the
    decoder runs out of data (NTK_JPEG_STATUS_TRUNCATED)."""
    data = encode(image(40, 72, "noise", 3), quality=90, subsampling=2)
    start = parse(data)["scan_start"]
    return data[:start + int(0.4 * (len(data) - start))]


# ------------------------------------------------------------------------------------------------------------------------------
# the device entry with guard bytes around every rectangle (GPU tests)
# ------------------------------------------------------------------------------------------------------------------------------

GUARD = 0xA5


def decode_guarded(cuda, files, rects, gap=96):
    """ntk_jpeg_decode_batch into a buffer filled with GUARD, `gap` bytes before, between and after the rectangles.
    -> (list of decoded rectangles, status, True when every byte outside the rectangles is still GUARD)"""
    import torch
    from ntmtrack import _lib, data
    probed = [data._probe_frame(f, "file %d" % i) for i, f in enumerate(files)]
    rects = [(0, 0) + pr["size"] if r is None else r for pr, r in zip(probed, rects)]
    packed = data.pack_jpeg_frames(probed, rects, staging=data.Staging())
    assert all(packed.jpeg.on_device)
    table = packed.table.numpy().copy()
    table[:, 0] += gap * (1 + np.arange(len(files)))
    total = packed.nbytes + gap * (len(files) + 1)
    pix = torch.full((total,), GUARD, dtype=torch.uint8, device=cuda)
    j, st, n = packed.jpeg, packed.staging, packed.n
    dev = lambda t: t.to(cuda)
    streams, descs, segs = dev(st.streams[:j.stream_bytes]), dev(st.descs[:n]), dev(st.segments[:j.n_segments])
    tab, ws = dev(torch.from_numpy(table)), torch.empty((j.workspace_bytes,), dtype=torch.uint8, device=cuda)
    status = torch.full((n,), 77, dtype=torch.int32, device=cuda)
    P = _lib.ptr
    _lib.check(_lib.lib().ntk_jpeg_decode_batch(P(streams), j.stream_bytes, P(descs), P(segs), j.n_segments, P(tab), P(pix), total,
                                                P(ws), j.workspace_bytes, P(status), n, _lib.stream()), "ntk_jpeg_decode_batch")
    torch.cuda.synchronize()
    out = pix.cpu().numpy()
    keep = np.ones(total, bool)
    images = []
    for off, _H, _W, _y0, _x0, h, w in table.tolist():
        images.append(out[off:off + h * w * 3].reshape(h, w, 3).copy())
        keep[off:off + h * w * 3] = False
    return images, status.cpu().numpy(), bool(np.all(out[keep] == GUARD))
