"""A baseline JPEG writer for the tests, pure Python / NumPy and independent of Pillow and of the project's C code (jpeg_util is used
for NATURAL only): coefficients in, file bytes out, with every table index, Huffman table shape, restart interval and marker layout
the device decoder accepts -- most of which Pillow's encoder never produces -- and the fixed, named, seeded corpus the JPEG tests
share (corpus()).

A corpus file must be one on which jpeg_util.decode equals Pillow (tests/test_jpeg_host.py asserts it per file): libjpeg-turbo's
SIMD inverse DCT saturates 16-bit intermediates where the restatement and the device keep int32, so the generators keep dequantised
coefficients within what a forward DCT of 8-bit samples gives (|DC| <= 1024, one large AC value per block at most)."""
import collections

import numpy as np

from jpeg_util import NATURAL

SAMPLINGS = {"gray": (1, 1, 1), "s444": (3, 1, 1), "s422": (3, 2, 1), "s420": (3, 2, 2)}      # name -> (components, hs, vs)

# ISO/IEC 10918-1 Annex K.3: (codes per length 1..16, values in code order)
_AC_TAIL = [(r << 4) | s for r in range(16) for s in range(1, 11)]
STD_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
STD_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
STD_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
    0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9,
    0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2,
    0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
STD_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17,
    0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
    0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7,
    0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2,
    0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
assert sorted(STD_AC_LUMA[1]) == sorted(STD_AC_CHROMA[1]) == sorted(_AC_TAIL + [0x00, 0xF0])


# ------------------------------------------------------------------------------------------------------------------------------
# coefficients -> symbols
# ------------------------------------------------------------------------------------------------------------------------------

def grid_shape(H, W, sampling):
    """-> (mcus_y, mcus_x, blocks per MCU)"""
    nc, hs, vs = SAMPLINGS[sampling]
    return -(-H // (8 * vs)), -(-W // (8 * hs)), (hs * vs + 2 if nc == 3 else 1)


def _size(v):
    return int(abs(int(v))).bit_length()


def _bits(v, s):
    """the s extra bits of a value of size s"""
    return v if v >= 0 else v + (1 << s) - 1


def tokens(coef, sampling, restart=0):
    """coef [mcus_y, mcus_x, blocks_per_mcu, 64] natural order -> one list per restart segment of (component, class, symbol,
    extra bits, number of extra bits), in coding order; the DC predictors restart with every segment."""
    nc, hs, vs = SAMPLINGS[sampling]
    nluma = hs * vs
    flat = np.asarray(coef).reshape(-1, coef.shape[2], 64)
    assert flat.shape[1] == (nluma + 2 if nc == 3 else 1)
    interval = restart if restart > 0 else len(flat)
    segments = []
    for m, mcu in enumerate(flat):
        if m % interval == 0:
            segments.append([])
            pred = [0, 0, 0]
        out = segments[-1]
        for b, blk in enumerate(mcu):
            c = 0 if b < nluma else b - nluma + 1
            z = [int(v) for v in blk[NATURAL]]
            d = z[0] - pred[c]
            pred[c] = z[0]
            s = _size(d)
            assert s <= 11, "DC difference %d" % d
            out.append((c, 0, s, _bits(d, s), s))
            run = 0
            for k in range(1, 64):
                if z[k] == 0:
                    run += 1
                    continue
                while run > 15:
                    out.append((c, 1, 0xF0, 0, 0))
                    run -= 16
                s = _size(z[k])
                assert s <= 10, "AC value %d" % z[k]
                out.append((c, 1, (run << 4) | s, _bits(z[k], s), s))
                run = 0
            if run:
                out.append((c, 1, 0x00, 0, 0))
    return segments


def frequencies(segments, comp_huff):
    """-> {(class, table index): Counter of symbols} for components that read tables comp_huff[c] = (td, ta)"""
    freq = collections.defaultdict(collections.Counter)
    for seg in segments:
        for c, cls, sym, _v, _n in seg:
            freq[(cls, comp_huff[c][cls])][sym] += 1
    return freq


def stats(coef, sampling, restart=0):
    """What a file's entropy stream exercises: sets of DC differences, AC values, (run, size) pairs, the numbers of ZRL met in a
    row before a coefficient, and counts of blocks that end at index 63, are all zero, or are DC only."""
    st = {"dc_diff": set(), "ac_value": set(), "run_size": set(), "zrl_rows": set(), "no_eob": 0, "zero_blocks": 0, "dc_only": 0}
    for seg in tokens(coef, sampling, restart):
        zrl = 0
        for _c, cls, sym, v, n in seg:
            val = (v if v >= (1 << (n - 1)) else v - (1 << n) + 1) if n else 0
            if cls == 0:
                st["dc_diff"].add(val)
            elif sym == 0xF0:
                zrl += 1
            elif sym:
                st["ac_value"].add(val)
                st["run_size"].add((sym >> 4, sym & 15))
                if zrl:
                    st["zrl_rows"].add(zrl)
                zrl = 0
    flat = np.asarray(coef).reshape(-1, 64)
    ac = np.delete(flat, 0, axis=1)
    st["no_eob"] = int(np.count_nonzero(flat[:, 63]))
    st["zero_blocks"] = int(np.count_nonzero(~flat.any(axis=1)))
    st["dc_only"] = int(np.count_nonzero((flat[:, 0] != 0) & ~ac.any(axis=1)))
    return st


# ------------------------------------------------------------------------------------------------------------------------------
# Huffman tables: (counts[16], values in code order)
# ------------------------------------------------------------------------------------------------------------------------------

def _from_lengths(lengths):
    """{symbol: code length} -> (counts, values): shorter codes first, symbols of one length in rising order"""
    order = sorted(lengths, key=lambda s: (lengths[s], s))
    counts = [0] * 16
    for s in order:
        counts[lengths[s] - 1] += 1
    code = 0
    for l in range(1, 17):                              # the codes fit and the all-ones code of 16 bits stays free
        code = (code + counts[l - 1]) << 1
        assert code <= (1 << (l + 1)) - (2 if l == 16 else 0), "the code lengths %s do not fit" % (counts,)
    return counts, order


def single_code_table(symbol):
    """one code, '0'"""
    return [1] + [0] * 15, [symbol]


def chain_table(freq, full=False):
    """Over just the symbols of `freq`: one code of each length 16, 15, ..., the most frequent symbol the longest, so that most
    symbols a decoder reads take its search over lengths 9..16 and not an 8-bit lookup.  Beyond 16 symbols the 8 most frequent take
    lengths 16..9 and the others share the shortest length that has room for them.  full (AC tables): run/size symbols the file
    does not use take the short lengths down to 1, so that the codes in use are rows of ones ended by a zero."""
    order = sorted(freq, key=lambda s: (-freq[s], s))
    if full:
        order += [s for s in reversed(_AC_TAIL) if s not in freq][:max(0, 16 - len(order))]
    if len(order) <= 16:
        return _from_lengths({s: 16 - i for i, s in enumerate(order)})
    rest = len(order) - 8
    L = max(1, int(rest).bit_length())                  # rest <= 2^L - 1: one code of length L is left for the longer ones
    lengths = {s: 16 - i for i, s in enumerate(order[:8])}
    lengths.update({s: L for s in order[8:]})
    return _from_lengths(lengths)


def frequency_table(freq, skew=False):
    """Huffman's construction limited to 16 bits the way Annex K.2 does it (a reserved symbol keeps the all-ones code free).
    skew: replace the counts by Fibonacci numbers in the order of frequency (the 30 most frequent symbols; 1 for the others), so
    that the unlimited code has lengths far beyond 16 bits and the limiting step has work to do."""
    freq = dict(freq)
    if skew:
        fib = [1, 2]
        while len(fib) < 31:
            fib.append(fib[-1] + fib[-2])
        for r, s in enumerate(sorted(freq, key=lambda s: (-freq[s], s))):
            freq[s] = fib[max(0, 30 - r)]
    f = {s: int(n) for s, n in freq.items() if n > 0}
    f[256] = 1
    size = {s: 0 for s in f}
    others = {s: -1 for s in f}
    while True:
        live = sorted((n, -s) for s, n in f.items() if n > 0)          # least frequent first, the larger symbol on ties
        if len(live) < 2:
            break
        c1, c2 = -live[0][1], -live[1][1]
        f[c1] += f[c2]
        f[c2] = 0
        for c, tail in ((c1, c2), (c2, None)):                          # every symbol of both trees gets one bit longer
            size[c] += 1
            while others[c] >= 0:
                c = others[c]
                size[c] += 1
            if tail is not None:
                others[c] = tail
    bits = [0] * 260
    for s in size:
        bits[size[s]] += 1
    longest = max(l for l in range(260) if bits[l])
    for i in range(longest, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                                        # the reserved symbol
    order = sorted((s for s in size if s != 256), key=lambda s: (size[s], s))
    counts = bits[1:17]
    assert sum(counts) == len(order)
    code = 0
    for l in range(1, 17):                                              # the codes fit
        code = (code + counts[l - 1]) << 1
        assert code <= (1 << (l + 1)) - (2 if l == 16 else 0), counts
    if skew and len(order) > 17:
        assert longest > 16, "the skewed counts were meant to need the 16-bit limit"
    return counts, order


def _encoder(table):
    """(counts, values) -> {symbol: (code, length)}"""
    counts, vals = table
    enc, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            enc[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return enc


# ------------------------------------------------------------------------------------------------------------------------------
# the file
# ------------------------------------------------------------------------------------------------------------------------------

def write(coef, H, W, sampling, quant, comp_quant, huff, comp_huff, restart=0, fill=False, merge_tables=False, dri_twice=False,
          decoy_dht=False, decoy_dqt=False, extras=False, ids=(1, 2, 3), jfif=True, pad_ones=True):
    """coef [mcus_y, mcus_x, blocks_per_mcu, 64] in natural order; quant {index 0..3: [64] natural order} and comp_quant[c] the
    index component c uses; huff {(class, index 0..3): (counts, values)} and comp_huff[c] = (DC index, AC index); restart: the
    interval in MCUs (0: none).  Layout: `fill` puts an FF before every marker of the header, every RSTn and EOI; `merge_tables`
    writes all DQT tables in one segment and all DHT tables in one (else one segment each); `dri_twice` writes a DRI with another
    interval first (1, or 2 beside an interval of 1: a decoder that keeps it expects other segments; the last one counts);
    `decoy_dht` / `decoy_dqt` define one table twice, first with other content;
    `extras` adds COM and APP1 segments; `ids` are the component ids; `jfif` writes the APP0 segment; `pad_ones` pads every
    segment's last byte with ones (the standard) or zeros.  -> file bytes"""
    nc, hs, vs = SAMPLINGS[sampling]
    assert tuple(coef.shape) == grid_shape(H, W, sampling) + (64,), (coef.shape, grid_shape(H, W, sampling))
    assert jfif or tuple(ids) == (1, 2, 3) or nc == 1
    pre = b"\xff" if fill else b""

    def seg(marker, body):
        return pre + bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)

    def dqt(t, q):
        q = np.asarray(q)
        assert q.shape == (64,) and q.min() >= 1 and q.max() <= 255
        return bytes([t]) + bytes(int(v) for v in q[NATURAL])

    def dht(key, table):
        counts, vals = table
        return bytes([(key[0] << 4) | key[1]]) + bytes(counts) + bytes(vals)

    out = [b"\xff\xd8"]
    if jfif:
        out.append(seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"))
    if extras:
        out.append(seg(0xFE, b"written by tests/jpeg_write.py"))
        out.append(seg(0xE1, b"ntk:synthetic\x00" + bytes(range(40))))
    if dri_twice:
        out.append(seg(0xDD, [0, 2 if restart == 1 else 1]))
    qkeys = sorted(quant)
    if decoy_dqt:
        t = comp_quant[0]
        out.append(seg(0xDB, dqt(t, (np.asarray(quant[t]) + 16) % 255 + 1)))
    if merge_tables:
        out.append(seg(0xDB, b"".join(dqt(t, quant[t]) for t in qkeys)))
    else:
        out += [seg(0xDB, dqt(t, quant[t])) for t in qkeys]
    if extras:
        out.append(seg(0xFE, b"between the tables"))
    sof = [8, H >> 8, H & 255, W >> 8, W & 255, nc]
    for c in range(nc):
        sof += [ids[c], ((hs << 4) | vs) if c == 0 and nc == 3 else 0x11, comp_quant[c]]
    out.append(seg(0xC0, sof))
    hkeys = sorted(huff)
    if decoy_dht:
        key = max(hkeys, key=lambda k: (len(huff[k][1]), k))            # the table with the most symbols, its values reversed
        assert len(set(huff[key][1])) > 1
        out.append(seg(0xC4, dht(key, (huff[key][0], huff[key][1][::-1]))))
    if merge_tables:
        out.append(seg(0xC4, b"".join(dht(k, huff[k]) for k in hkeys)))
    else:
        out += [seg(0xC4, dht(k, huff[k])) for k in hkeys]
    if restart or dri_twice:
        out.append(seg(0xDD, [restart >> 8, restart & 255]))
    sos = [nc]
    for c in range(nc):
        sos += [ids[c], (comp_huff[c][0] << 4) | comp_huff[c][1]]
    out.append(seg(0xDA, sos + [0, 63, 0]))
    enc = {k: _encoder(t) for k, t in huff.items()}
    for n, segment in enumerate(tokens(coef, sampling, restart)):
        if n:
            out.append(pre + bytes([0xFF, 0xD0 + ((n - 1) & 7)]))
        acc, nbits = 0, 0
        for c, cls, sym, v, nv in segment:
            code, l = enc[(cls, comp_huff[c][cls])][sym]
            acc = (((acc << l) | code) << nv) | v
            nbits += l + nv
        pad = -nbits % 8
        acc = (acc << pad) | (((1 << pad) - 1) if pad_ones else 0)
        out.append(acc.to_bytes((nbits + pad) // 8, "big").replace(b"\xff", b"\xff\x00"))
    out.append(pre + b"\xff\xd9")
    return b"".join(out)


def tables_for(coef, sampling, restart, comp_huff, kind):
    """Huffman tables for the symbols the file uses: kind "chain" / "frequency" / "skewed" per (class, index) that comp_huff names;
    "ones": chain tables whose AC codes in use are rows of ones"""
    build = {"chain": lambda k, f: chain_table(f), "frequency": lambda k, f: frequency_table(f),
             "skewed": lambda k, f: frequency_table(f, skew=True), "ones": lambda k, f: chain_table(f, full=k[0] == 1)}[kind]
    return {k: build(k, f) for k, f in frequencies(tokens(coef, sampling, restart), comp_huff).items()}


# ------------------------------------------------------------------------------------------------------------------------------
# coefficient generators
# ------------------------------------------------------------------------------------------------------------------------------

_DCT = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


def _blocks(plane, q):
    """plane [8a, 8b] float samples -> quantised coefficients [a, b, 64] natural order"""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    x = (plane - 128.0).reshape(a, 8, b, 8).transpose(0, 2, 1, 3)
    c = np.einsum("ux,abxy,vy->abuv", _DCT, x, _DCT).reshape(a, b, 64)
    return np.rint(c / np.asarray(q, np.float64)).astype(np.int64)


def from_image(img, sampling, quant, comp_quant):
    """uint8 [H, W, 3] (or [H, W] for "gray") -> coefficients: JFIF's YCbCr, chroma averaged over hs x vs, edges replicated out
    to whole MCUs, float DCT, rounding division by the component's table."""
    nc, hs, vs = SAMPLINGS[sampling]
    H, W = img.shape[:2]
    my, mx, bpm = grid_shape(H, W, sampling)
    f = np.pad(img.astype(np.float64), ((0, my * 8 * vs - H), (0, mx * 8 * hs - W)) + ((0, 0),) * (img.ndim - 2), mode="edge")
    if nc == 1:
        assert img.ndim == 2
        return _blocks(f, quant[comp_quant[0]]).reshape(my, mx, 1, 64)
    R, G, B = f[..., 0], f[..., 1], f[..., 2]
    Y = 0.299 * R + 0.587 * G + 0.114 * B
    Cb = -0.168736 * R - 0.331264 * G + 0.5 * B + 128
    Cr = 0.5 * R - 0.418688 * G - 0.081312 * B + 128
    sub = lambda p: p.reshape(my * 8, vs, mx * 8, hs).mean(axis=(1, 3))
    coef = np.zeros((my, mx, bpm, 64), np.int64)
    coef[:, :, :hs * vs] = _blocks(Y, quant[comp_quant[0]]).reshape(my, vs, mx, hs, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, hs * vs, 64)
    coef[:, :, hs * vs] = _blocks(sub(Cb), quant[comp_quant[1]])
    coef[:, :, hs * vs + 1] = _blocks(sub(Cr), quant[comp_quant[2]])
    return coef


def _component_blocks(coef, sampling):
    """-> per component the list of its blocks (views [64] into coef, zigzag-indexed through NATURAL by the caller) in coding order"""
    nc, hs, vs = SAMPLINGS[sampling]
    nluma = hs * vs
    flat = coef.reshape(-1, coef.shape[2], 64)
    comps = [[] for _ in range(nc)]
    for mcu in flat:
        for b in range(mcu.shape[0]):
            comps[0 if b < nluma else b - nluma + 1].append(mcu[b])
    return comps


def dc_walk():
    """DC values whose successive differences (from 0) are 0 and both ends, with both signs, of every category 1..11:
    +-2^(s-1) and +-(2^s - 1); every value stays within [-1024, 1023], what 8-bit samples give at a quantiser of 1."""
    todo = [0] + [sg * v for s in range(11, 0, -1) for v in ((1 << s) - 1, 1 << (s - 1)) for sg in (1, -1)]
    todo = list(dict.fromkeys(todo))
    seq, dc = [], 0
    while todo:
        fit = [d for d in todo if -1024 <= dc + d <= 1023]
        if fit:
            d = fit[0]
            todo.remove(d)
        else:
            d = (-1024 - dc) if todo[0] > 0 else (1023 - dc)            # go to the end from which the next one fits
        dc += d
        seq.append(dc)
    return seq


def field_dc_walk(H, W, sampling):
    """DC-only blocks along dc_walk() in every component (as far as the component has blocks), all-zero blocks behind."""
    coef = np.zeros(grid_shape(H, W, sampling) + (64,), np.int64)
    walk = dc_walk()
    comps = _component_blocks(coef, sampling)
    assert len(comps[0]) >= len(walk) + 2, "the luma component has %d blocks for %d steps" % (len(comps[0]), len(walk))
    for c, blocks in enumerate(comps):
        for blk, v in zip(blocks, walk[::1 if c == 0 else -1]):         # chroma walks it backwards: other values meet
            blk[0] = v
    return coef


AC_ENDS = [sg * v for s in range(1, 11) for v in (1 << (s - 1), (1 << s) - 1) for sg in (1, -1)]


def field_ac_ends(H, W, sampling, seed):
    """One AC_ENDS value per block after a run of 0..15 zeros (block j of a component: run j % 16), then -- where it fits -- a
    small value behind one, two or three ZRL, and in every seventh block a value at index 63 (no EOB).  Small DC values."""
    rng = np.random.default_rng(seed)
    coef = np.zeros(grid_shape(H, W, sampling) + (64,), np.int64)
    for c, blocks in enumerate(_component_blocks(coef, sampling)):
        for j, blk in enumerate(blocks):
            blk[0] = int(rng.integers(-40, 41))
            k = 1 + j % 16
            blk[NATURAL[k]] = AC_ENDS[(j + 13 * c) % len(AC_ENDS)]
            z = j % 4
            k2 = k + 1 + 16 * z + int(rng.integers(0, 3))
            if z and k2 <= 63:
                blk[NATURAL[k2]] = int(rng.choice([-2, -1, 1, 2]))
            if j % 7 == 3:
                blk[63] = int(rng.choice([-1, 1]))
    return coef


def field_runs(H, W, sampling, seed):
    """Small values (|v| <= 7) at gaps that take every run 0..15, with one, two and three ZRL before a coefficient, blocks that
    end at index 63, and now and then an all-zero or a DC-only block."""
    rng = np.random.default_rng(seed)
    coef = np.zeros(grid_shape(H, W, sampling) + (64,), np.int64)
    for c, blocks in enumerate(_component_blocks(coef, sampling)):
        for j, blk in enumerate(blocks):
            if j % 11 == 5:
                continue                                               # all zero
            blk[0] = int(rng.integers(-60, 61)) or 1
            if j % 11 == 7:
                continue                                               # DC only
            k, i = 1, 0
            while True:
                gap = (j * 7 + i * 5 + c) % 16
                if i == 1 and j % 3 == 0:
                    gap += 16 * (1 + (j // 3) % 3)
                k += gap
                if k > 63:
                    break
                blk[NATURAL[k]] = int(rng.choice([-1, 1])) * (1 + (i + j) % 7)
                k += 1
                i += 1
            if j % 5 == 0:
                blk[63] = int(rng.choice([-3, 3]))
    return coef


def field_all_ones(H, W, sampling, seed):
    """Values whose extra bits are all ones (2^s - 1): the DC of every block is one of them, AC values at indices 1..12 and 255
    at index 63, so every block -- and with restart interval 1 every segment -- ends in eight one bits or more: the last byte
    before each restart marker is a stuffed FF."""
    rng = np.random.default_rng(seed)
    coef = np.zeros(grid_shape(H, W, sampling) + (64,), np.int64)
    for c, blocks in enumerate(_component_blocks(coef, sampling)):
        dc = (1 << int(rng.integers(4, 8))) - 1
        for j, blk in enumerate(blocks):
            blk[0] = dc
            for i in range(1, 13):
                blk[NATURAL[i]] = (1 << (1 + (i + j + c) % 5)) - 1
            blk[63] = 255
    return coef


def field_small_times_255(H, W, sampling, seed):
    """DC 0 everywhere (a single-code DC table serves), +-1 / +-2 at one of the indices 1..5 -- where quant_255() is 255 -- and a
    small value further on."""
    rng = np.random.default_rng(seed)
    coef = np.zeros(grid_shape(H, W, sampling) + (64,), np.int64)
    for c, blocks in enumerate(_component_blocks(coef, sampling)):
        for j, blk in enumerate(blocks):
            blk[NATURAL[1 + (j + c) % 5]] = int(rng.choice([-2, -1, 1, 2]))
            blk[NATURAL[10 + j % 7]] = int(rng.choice([-3, -2, 2, 3]))
    return coef


def quant_ones():
    return np.ones(64, np.int64)


def quant_255():
    q = np.full(64, 12, np.int64)
    q[NATURAL[1:6]] = 255
    return q


def quant_ramp(base, step):
    u, v = np.mgrid[0:8, 0:8]
    return np.clip(base + step * (u + v), 1, 255).reshape(64).astype(np.int64)


def picture(H, W, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    ph = rng.uniform(0, 6.28, size=3)
    img = [127.5 + 150 * np.sin(ph[c] + x * (0.13 + 0.06 * c) + y * (0.09 + 0.04 * c)) for c in range(3)]
    return np.clip(np.stack(img, axis=-1), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------------
# the corpus
# ------------------------------------------------------------------------------------------------------------------------------

MANY_SEGMENTS = {"gray": (160, 200, 2), "s444": (88, 96, 1), "s422": (88, 192, 1), "s420": (176, 192, 1)}   # H, W, interval


def _std(comp_huff):
    std = {(0, 0): STD_DC_LUMA, (1, 0): STD_AC_LUMA, (0, 1): STD_DC_CHROMA, (1, 1): STD_AC_CHROMA}
    return {(cls, t[cls]): std[(cls, t[cls])] for t in comp_huff for cls in (0, 1)}


def _recipes(sampling):
    """-> list of (name, dict of write()'s arguments); every recipe exists for every sampling"""
    nc, hs, vs = SAMPLINGS[sampling]
    sd = list(SAMPLINGS).index(sampling)
    per = lambda *v: tuple(v[:nc])
    pic = lambda H, W, kind, seed: picture(H, W, kind, seed) if nc == 3 else picture(H, W, kind, seed)[:, :, 1].copy()
    out = []

    def add(name, H, W, coef, quant, comp_quant, comp_huff, huff, restart=0, **layout):
        if isinstance(huff, str):
            huff = tables_for(coef, sampling, restart, comp_huff, huff)
        out.append(("%s_%s_%dx%d" % (sampling, name, H, W),
                    dict(coef=coef, H=H, W=W, sampling=sampling, quant=quant, comp_quant=comp_quant, huff=huff, comp_huff=comp_huff,
                         restart=restart, **layout)))

    # DC differences at both ends of every category; DC-only and all-zero blocks; one standard table pair shared by all components;
    # quantisation all ones; the plain layout
    H, W = 64, 80
    shared = per((0, 0), (0, 0), (0, 0))
    add("dcwalk", H, W, field_dc_walk(H, W, sampling), {0: quant_ones()}, per(0, 0, 0), shared, _std(shared))
    # AC values at both ends of every size, every run, ZRL rows, index 63; chain tables at indices 2 and 3; quantisation tables 2 and
    # 3; restart interval = the MCU count; every layout switch away from the default
    H, W = 48, 64
    my, mx, _ = grid_shape(H, W, sampling)
    add("acends", H, W, field_ac_ends(H, W, sampling, 11 + sd), {3: quant_ones(), 2: quant_ones()}, per(3, 2, 2),
        per((2, 3), (3, 2), (3, 2)), "chain", restart=my * mx, fill=True, merge_tables=True, dri_twice=True, decoy_dht=True,
        decoy_dqt=True, extras=True, ids=(0, 1, 2), pad_ones=False)
    # every run, ZRL rows, index 63, zero and DC-only blocks; skewed frequency tables (the 16-bit limit at work); an interval that
    # divides neither a row nor the frame; fill bytes before RSTn; no JFIF segment
    H, W = 33, 47
    add("runs", H, W, field_runs(H, W, sampling, 23 + sd), {0: quant_ramp(1, 0), 1: quant_ramp(2, 0)}, per(0, 1, 1),
        per((0, 0), (1, 1), (1, 1)), "skewed", restart=7, fill=True, jfif=False, extras=True, dri_twice=True)
    # all-ones extra bits, FF 00 everywhere, a stuffed FF before every RSTn; interval 1; chain tables; with and without fill bytes
    add("ones", 17, 23, field_all_ones(17, 23, sampling, 31 + sd), {0: quant_ones()}, per(0, 0, 0), per((0, 0), (1, 1), (1, 1)),
        "ones", restart=1)
    add("onesfill", 16, 16, field_all_ones(16, 16, sampling, 37 + sd), {1: quant_ones()}, per(1, 1, 1), per((1, 1), (1, 1), (1, 1)),
        "ones", restart=1, fill=True, merge_tables=True, pad_ones=False)
    # a DC that never changes under a single-code DC table; 255 in the quantisation table under small coefficients; an interval
    # larger than the MCU count, after a decoy DRI
    H, W = 40, 72
    dc0 = per((2, 0), (2, 0), (2, 0))
    add("dc0q255", H, W, field_small_times_255(H, W, sampling, 41 + sd), {1: quant_255()}, per(1, 1, 1), dc0,
        {(0, 2): single_code_table(0), (1, 0): STD_AC_LUMA}, restart=1000, dri_twice=True)
    # pictures through the float DCT: three quantisation tables and three different (frequency-built) Huffman table pairs for three
    # components, merged table segments, both decoys, ids 0 1 2, zero padding
    H, W = 33, 47
    q3 = {3: quant_ramp(1, 1), 1: quant_ramp(2, 2), 2: quant_ramp(3, 3)}
    add("noise3", H, W, from_image(pic(H, W, "noise", 51), sampling, q3, per(3, 1, 2)), q3, per(3, 1, 2), per((0, 3), (1, 2), (2, 1)),
        "frequency", restart=3, merge_tables=True, decoy_dht=True, decoy_dqt=True, ids=(0, 1, 2), pad_ones=False)
    H, W = 17, 23
    add("smooth3", H, W, from_image(pic(H, W, "smooth", 53), sampling, q3, per(3, 1, 2)), q3, per(3, 1, 2),
        per((3, 0), (2, 1), (1, 2)), "frequency", jfif=False, extras=True)
    # more than 128 restart segments in one frame (the entropy kernel's lane loop takes a third trip)
    H, W, interval = MANY_SEGMENTS[sampling]
    qm = {0: quant_ramp(6, 5), 1: quant_ramp(9, 8)}
    luma_chroma = per((0, 0), (1, 1), (1, 1))
    add("manyseg", H, W, from_image(pic(H, W, "smooth", 59), sampling, qm, per(0, 1, 1)), qm, per(0, 1, 1), luma_chroma,
        _std(luma_chroma), restart=interval)
    return out


def recipes():
    """-> list of (name, write()'s arguments) for the whole corpus, in its fixed order"""
    return [r for sampling in SAMPLINGS for r in _recipes(sampling)]


_CORPUS = []


def corpus():
    """The synthetic corpus: (name, file bytes), like jpeg_util.grid().  Fixed, named and seeded; built once per process."""
    if not _CORPUS:
        _CORPUS.extend((name, write(**kw)) for name, kw in recipes())
    return list(_CORPUS)
