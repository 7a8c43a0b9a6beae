"""GPU: the stand-alone DNC module kernels (csrc/dnc_modules.hip) and NTM ops (csrc/ntm_ops.hip) at the sizes where their strided
loops take a second step, against oracle/dnc_oracle.py and oracle/ntm_oracle.py evaluated in float64.

The C entries are called directly (ntmtrack._lib.lib()) with device pointers: MemoryAccess pads the word size to a multiple of 4
and reshapes, which would remove half of these cases.  Every output starts as GUARD_NAN inside a buffer with guard words on both
sides (small_kernel_util.FlatGuarded): after the call no output element is NaN and the guards hold their bits.  Every operand is
surrounded by INPUT_NAN, `raw` has ldr = I + 5 with INPUT_NAN in the padding: a read past an operand's end makes a NaN that is not
the guard's.  Each case has B >= 2 (unless the table says otherwise) with different data per batch element.

kernel (block)                 case                                   the loop or limit it sits on
cosine_weights_kernel (256)    N 1, 63, 64, 65, 130 x H 1, 4, 5, 9    `n = lane; n += 64` takes 1 / 1 / 1 / 2 / 3 steps; `h = wave; h += 4` takes
                                                                      1 / 1 / 2 / 3 steps; N = 1, H = 1, W = 1 the minimum; H N up to 1170 > 256
                               H 16, N 1024, W 4, B 1                 H N = 16384 scores = the 64 KiB of LDS the launcher accepts
                               zero row and zero key                  the EPS form: 0 / (sqrt(EPS) sqrt(EPS) + EPS), finite
                               strengths in [-5, 20]                  the max subtraction of the softmax
linkage_kernel (256)           N 1, 17, 64, 255, 256, 257, 300        red[] holds 1 / 1 / 1 / 4 / 4 / 4 / 4 non-empty wave sums; N N up to 90000 > 256;
                               x Wn 1, 3                              at N >= 256 each 64-slot quarter of ww carries weight (asserted on the oracle)
directional_kernel (256)       N 1, 255, 256, 257, both directions    `n += 256` takes a second step at 257; R = 3 != Wn = 2 pins brj's decomposition
freeness_kernel (256)          N 1, 256, 257, Wn 3, R 2               second step at 257 (the planted slots are the last ones)
allocation_kernel (1024)       N 1, 2, 1023, 1024, 1025, 2050         `n += 1024` takes 1 / 1 / 1 / 1 / 2 / 3 steps
                               x Wn 1 (write_gates null), 3
                               N 8192, Wn 1, B 1                      2 N floats = the 64 KiB of LDS the launcher accepts; 8 steps
                               ties at N 1100: two, three, all-zero,  `num == nun && m < n` across the stride (a tied pair sits in different steps)
                               all-one usage
interface_act_kernel (256)     (W, R, Wn) = (1, 1, 1)                 I = 12, the minimum
                               (20, 4, 2), (24, 4, 2), (64, 4, 4)     I = 234 / 274 / 1080: `c += 256` takes 1 / 2 / 5 steps
gate_product / write_mix /     ntk_dnc_write_weights and              N = 260 > 256 threads per (batch, head) block; (2, 1, 1, 1, 1) the minimum;
read_mix kernels (256)         ntk_dnc_read_weights, (B, N, W, R, Wn)  B Wn = 260 > 256: gate_product_kernel's second block
                               = (2, 260, 20, 3, 2), (2, 1, 1, 1, 1),
                               (130, 3, 2, 2, 2)
erase_write_kernel (1024)      N x W = 33 x 31, 32 x 32, 41 x 25,     N W = 1023 / 1024 / 1025 / 2600
                               130 x 20, Wn 3; 1 x 1
read_words_kernel (128)        W 1, 127, 128, 129, R 3                `w += 128` takes a second step at 129
ntk_dnc_access_step_fwd        (N, W, R, Wn) = (260, 20, 4, 2),       three chained steps, all of the above composed; W = 132 > 128
                               (64, 132, 2, 1)
ntk_dnc_access_step_bwd        (64, 16, 4, 4), (128, 20, 4, 2)        R = Wn = 4 its limits; I = 312 / 234 (IP = 236): ifc_rows_kernel and
(ifc_rows, access_carry)                                              access_carry_kernel run a grid of 3 / 2 and 8 / 5 blocks of 256
cosine_similarity_kernel (256) N 1, 63, 257 x Md 1, 20, 300           Md = 300: the column-scale loop `m += 256` takes a second step; H N = 1285
                               x H 1, 5, both modes; zero row,
                               zero column, zero key
circular_convolution_kernel    N 1, 2, 3, 255, 256, 257               `i += 256` second step at 257; even SS pins start = floor(-SS / 2); SS = N wraps
(256)                          x SS 1, 2, 3, 4, 5, N (SS <= N)        every tap; a one-hot kernel on tap j = circular_shift by j's offset, bit for bit

Bounds.  floor = the bound tests/test_modules_gpu.py states for the quantity: 1e-5 cosine weights, 1e-6 allocation and
directional reads, 2e-6 write weights, 2e-5 read weights and everything a composed step returns, 2e-6 NTM cosine similarity, 1e-6
circular convolution.  Quantities without a stated bound (linkage, precedence, usage, interface activations, erase-and-write,
read words) are a handful of float32 roundings of values of magnitude <= 1 (memory: <= 4): floor 1e-6 (erase-and-write and read
words: 2e-5, the bound of a step's memory and read words).  A case's bound is max(floor, 3 x the float32 numpy oracle's own
distance from the float64 oracle on the same inputs), computed in the test from the oracles alone; allocation and NTM circular
convolution use the floor alone.  oracle_side() evaluates every case without a device.  Largest float32-vs-float64 distances it
reports (3 x the distance stays below the floor in every case of today's table, so every bound in force is its floor):

    cosine_weights 7.1e-07 (the strengths-up-to-20 case)   linkage 5.1e-08   directional 2.8e-09   freeness 1.1e-07
    allocation 3.5e-08 (a quarter of its bound: 2.5e-07)   interface 8.6e-08   write_weights 1.1e-07   read_weights 4.3e-08
    erase_and_write 5.4e-07   read_words 3.0e-07   access_step_fwd 6.7e-07 (three steps)   ntm_cosine_similarity 2.1e-07
    ntm_circular_convolution 3.3e-08

(`PYTHONPATH=. python tests/test_module_shapes_gpu.py` prints them, without a device; replace them when a case or a seed changes.)"""
import functools

import numpy as np
import pytest
import torch

from oracle import dnc_oracle as D
from oracle import dnc_oracle_torch as DT
from oracle import ntm_oracle as O
from small_kernel_util import FlatGuarded, GUARD_NAN, Guarded, INPUT_NAN, raw_bytes_equal

pytestmark = pytest.mark.gpu

BAD_PTR = -2
f64 = lambda a: np.asarray(a, np.float64)
OWN = {}          # kernel family -> largest float32-vs-float64 oracle distance seen (oracle_side() prints it)


def _bound(family, floor, o32, o64, rule=True):
    """max(floor, 3 x the float32 oracle's own distance from the float64 one); the oracles alone decide it."""
    own = max(float(np.max(np.abs(f64(a) - b))) if b.size else 0.0 for a, b in zip(o32, o64))
    OWN[family] = max(OWN.get(family, 0.0), own)
    return max(floor, 3 * own) if rule else floor


def _rand_state(rng, B, N, W, R, Wn):
    """A non-degenerate access state (as test_memory_access_step_gradients_match_autograd builds it): distinct, well separated
    usages; read / write / precedence weights summing to less than 1; a random, NOT symmetric link with row and column sums at most
    1 and a zero diagonal."""
    f = lambda *s: rng.random(s).astype(np.float32)
    usage = (np.stack([rng.permutation(N) for _ in range(B)]).astype(np.float32) / N * 0.8 + 0.1).astype(np.float32)
    rw = f(B, R, N); rw /= rw.sum(2, keepdims=True) + 1
    ww = f(B, Wn, N); ww /= ww.sum(2, keepdims=True) + 1
    prec = f(B, Wn, N); prec /= prec.sum(2, keepdims=True) + 1
    link = f(B, Wn, N, N)
    link /= np.maximum(link.sum(2, keepdims=True), 1); link /= np.maximum(link.sum(3, keepdims=True), 1)
    link[:, :, np.arange(N), np.arange(N)] = 0
    return D.AccessState((f(B, N, W) - 0.5).astype(np.float32), rw, ww, D.TemporalLinkageState(link.astype(np.float32), prec), usage)


class Dev(object):
    """Operands on the device, each surrounded by INPUT_NAN; outputs prefilled with GUARD_NAN between guard words."""

    def __init__(self, cuda):
        from ntmtrack import _lib
        self.cuda, self.L, self.lib, self.st = cuda, _lib.lib(), _lib, _lib.stream()

    def inp(self, a):
        return FlatGuarded(np.shape(a), self.cuda, init=a)

    def out(self, *shape):
        return FlatGuarded(shape, self.cuda)

    def call(self, name, *args):
        self.lib.check(getattr(self.L, name)(*(tuple(getattr(a, "ptr", a) for a in args) + (self.st,))), name)
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def dev(cuda):
    return Dev(cuda)


def close(got, ref, bound, what=""):
    err = float(np.max(np.abs(f64(got) - ref))) if ref.size else 0.0
    assert err <= bound, "%s: max |kernel - float64 oracle| = %.3g > %.3g" % (what, err, bound)


# ------------------------------------------------------------------------------------------------------------ cosine weights
COS_W = (1, 3, 20)
COS_CASES = [(N, H, COS_W[(i + j) % 3], 2, "normal") for i, N in enumerate((1, 63, 64, 65, 130)) for j, H in enumerate((1, 4, 5, 9))]
COS_CASES += [(1024, 16, 4, 1, "normal"), (65, 5, 3, 2, "zeros"), (130, 5, 20, 2, "strong")]


@functools.lru_cache(maxsize=None)
def _cos_oracle(N, H, W, B, kind):
    rng = np.random.default_rng(1000 * N + 10 * H + W)
    mem = rng.standard_normal((B, N, W)).astype(np.float32)
    keys = rng.standard_normal((B, H, W)).astype(np.float32)
    s = (rng.uniform(-5, 20, (B, H)) if kind == "strong" else rng.standard_normal((B, H))).astype(np.float32)
    if kind == "zeros":
        mem[0, 3] = 0; mem[1, N - 1] = 0; keys[0, 1] = 0; keys[1, H - 1] = 0
    o64 = D.cosine_weights(f64(mem), f64(keys), f64(s))
    assert np.isfinite(o64).all()
    if kind == "strong":                # the scores of one row spread over more than e^10: the max subtraction carries weight
        assert np.log(o64.max(2) / np.maximum(o64.min(2), 1e-300)).max() > 10
    return mem, keys, s, o64, _bound("cosine_weights", 1e-5, [D.cosine_weights(mem, keys, s)], [o64])


@pytest.mark.parametrize("N,H,W,B,kind", COS_CASES, ids=lambda v: str(v))
def test_cosine_weights(dev, N, H, W, B, kind):
    mem, keys, s, o64, bound = _cos_oracle(N, H, W, B, kind)
    out = dev.out(B, H, N)
    dev.call("ntk_dnc_cosine_weights", dev.inp(mem), dev.inp(keys), dev.inp(s), out, B, N, W, H)
    got = out.written()
    close(got, o64, bound, "cosine weights")
    close(got.sum(2), np.ones((B, H)), 1e-5, "rows sum to 1")


# ------------------------------------------------------------------------------------------------------------------- linkage
@functools.lru_cache(maxsize=None)
def _linkage_oracle(N, Wn):
    B = 2
    rng = np.random.default_rng(100 * N + Wn)
    st = _rand_state(rng, B, N, 1, 1, Wn)
    link0, prec0, ww = st.linkage.link, st.linkage.precedence_weights, st.write_weights
    l64, p64 = D.link_update(f64(link0), f64(prec0), f64(ww)), D.precedence_weights(f64(prec0), f64(ww))
    bound = _bound("linkage", 1e-6, [D.link_update(link0, prec0, ww), D.precedence_weights(prec0, ww)], [l64, p64])
    if N >= 256:
        # the sum of the write weights is spread over the slots of all four waves (thread t sums slots t, t + 256, ...): without any
        # one wave's partial sum the precedence of the OTHER slots moves by more than the bound
        for q in range(4):
            mask = (np.arange(N) % 256) // 64 == q
            w0 = f64(ww).copy(); w0[:, :, mask] = 0
            moved = np.abs(D.precedence_weights(f64(prec0), w0) - p64)[:, :, ~mask]
            assert moved.max() > 10 * bound, (q, moved.max())
    return link0, prec0, ww, l64, p64, bound


@pytest.mark.parametrize("Wn", [1, 3])
@pytest.mark.parametrize("N", [1, 17, 64, 255, 256, 257, 300])
def test_linkage(dev, N, Wn):
    link0, prec0, ww, l64, p64, bound = _linkage_oracle(N, Wn)
    B = 2
    link, prec = dev.out(B, Wn, N, N), dev.out(B, Wn, N)
    dev.call("ntk_dnc_linkage", dev.inp(link0), dev.inp(prec0), dev.inp(ww), link, prec, B, N, Wn)
    gl, gp = link.written(), prec.written()
    close(gl, l64, bound, "link")
    close(gp, p64, bound, "precedence")
    diag = gl[:, :, np.arange(N), np.arange(N)]
    assert raw_bytes_equal(diag, np.zeros_like(diag)), "the diagonal of the link is +0.0 exactly"


# --------------------------------------------------------------------------------------------------------- directional reads
@functools.lru_cache(maxsize=None)
def _directional_oracle(N):
    B, R, Wn = 2, 3, 2
    st = _rand_state(np.random.default_rng(7 * N + 1), B, N, 1, R, Wn)
    link, prw = st.linkage.link, st.read_weights
    o64 = [D.directional_read_weights(f64(link), f64(prw), fw) for fw in (False, True)]
    bound = _bound("directional", 1e-6, [D.directional_read_weights(link, prw, fw) for fw in (False, True)], o64)
    if N > 1:           # (N = 1: the link is its own zero diagonal, both directions are 0)
        assert np.abs(o64[0] - o64[1]).max() > 100 * bound, "the link is not symmetric: the directions must differ"
    return link, prw, o64, bound


@pytest.mark.parametrize("forward", [0, 1], ids=["backward", "forward"])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_directional_read_weights(dev, N, forward):
    link, prw, o64, bound = _directional_oracle(N)
    B, R, Wn = 2, 3, 2
    out = dev.out(B, R, Wn, N)
    dev.call("ntk_dnc_directional_read_weights", dev.inp(link), dev.inp(prw), out, B, N, Wn, R, forward)
    close(out.written(), o64[forward], bound, "directional read weights")


# ------------------------------------------------------------------------------------------------------------------ freeness
@functools.lru_cache(maxsize=None)
def _freeness_oracle(N):
    B, Wn, R = 3, 3, 2
    rng = np.random.default_rng(3 * N + 2)
    st = _rand_state(rng, B, N, 1, R, Wn)
    ww, rw, pu = st.write_weights.copy(), st.read_weights.copy(), st.usage
    fg = rng.random((B, R)).astype(np.float32)
    # batch 1: the last slot was written with weight 1 by head 2 and no read head frees it -> usage exactly 1;
    # batch 2: read head 0 read the last slot with weight 1 and frees it with gate 1 -> usage exactly 0
    ww[1, 2, N - 1] = 1; rw[1, :, N - 1] = 0
    rw[2, 0, N - 1] = 1; fg[2, 0] = 1
    o64 = D.freeness(f64(ww), f64(fg), f64(rw), f64(pu))
    assert o64[1, N - 1] == 1 and o64[2, N - 1] == 0
    return ww, fg, rw, pu, o64, _bound("freeness", 1e-6, [D.freeness(ww, fg, rw, pu)], [o64])


@pytest.mark.parametrize("N", [1, 256, 257])
def test_freeness(dev, N):
    ww, fg, rw, pu, o64, bound = _freeness_oracle(N)
    B, Wn, R = 3, 3, 2
    out = dev.out(B, N)
    dev.call("ntk_dnc_freeness", dev.inp(ww), dev.inp(fg), dev.inp(rw), dev.inp(pu), out, B, N, Wn, R)
    got = out.written()
    close(got, o64, bound, "usage")
    assert got[1, N - 1] == 1.0 and got[2, N - 1] == 0.0
    assert got.min() >= 0 and got.max() <= 1


# ---------------------------------------------------------------------------------------------------------------- allocation
ALLOC_BOUND = 1e-6
ALLOC_CASES = [(N, Wn, 2) for N in (1, 2, 1023, 1024, 1025, 2050) for Wn in (1, 3)] + [(8192, 1, 1)]


def _alloc_check(usage, gates, Wn):
    """float64 oracle of a case, after the conditioning assertion: the float32 oracle agrees with it within a quarter of the bound
    (a near-tie would not: swapping two almost equal usages changes one allocation by a factor u)."""
    g = gates if gates is not None else np.zeros((usage.shape[0], Wn), np.float32)
    o32, o64 = D.write_allocation_weights(usage, g, Wn), D.write_allocation_weights(f64(usage), f64(g), Wn)
    own = float(np.max(np.abs(f64(o32) - o64)))
    OWN["allocation"] = max(OWN.get("allocation", 0.0), own)
    assert own <= ALLOC_BOUND / 4, "ill-conditioned allocation case (float32 vs float64 oracle %.3g): change the seed" % own
    return o64


@functools.lru_cache(maxsize=None)
def _alloc_oracle(N, Wn, B):
    rng = np.random.default_rng(11 * N + Wn)
    usage = (np.stack([rng.permutation(N) for _ in range(B)]).astype(np.float32) / N * 0.8 + 0.1).astype(np.float32)
    gates = rng.random((B, Wn)).astype(np.float32) if Wn > 1 else None
    return usage, gates, _alloc_check(usage, gates, Wn)


@pytest.mark.parametrize("N,Wn,B", ALLOC_CASES)
def test_allocation(dev, N, Wn, B):
    usage, gates, o64 = _alloc_oracle(N, Wn, B)
    out = dev.out(B, Wn, N)
    dev.call("ntk_dnc_write_allocation_weights", dev.inp(usage), dev.inp(gates) if gates is not None else None, out, B, N, Wn)
    close(out.written(), o64, ALLOC_BOUND, "allocation weights")


TIE_N = 1100          # > 1024: a tied pair (5, 1050) sits in different steps of the stride, (3, 700, 1099) in both


@functools.lru_cache(maxsize=None)
def _tie_oracle(kind):
    rng = np.random.default_rng(5)
    usage = (np.stack([rng.permutation(TIE_N) for _ in range(2)]).astype(np.float32) / TIE_N * 0.8 + 0.1).astype(np.float32)
    if kind == "two":
        usage[:, 1050] = usage[:, 5]
    elif kind == "three":
        usage[0, 700] = usage[0, 1099] = usage[0, 3]
        usage[1, 3] = usage[1, 700] = usage[1, 1099]
    elif kind == "zero":
        usage[:] = 0
    elif kind == "one":
        usage[:] = 1
    elif kind == "lowest_tied":          # the two least used slots are tied: the allocations at stake are 0.9 and 0.09
        usage[0, 1050] = usage[0, 5] = 0.05
        usage[1, 1024] = usage[1, 1023] = 0.05
    return usage, _alloc_check(usage, None, 1)


@pytest.mark.parametrize("kind", ["two", "three", "zero", "one", "lowest_tied"])
def test_allocation_breaks_exact_ties_by_lower_index(dev, kind):
    """A tie between float32 usages is a tie in both precisions: the oracle's stable sort puts the lower index first, so must the
    kernel's rank rule."""
    usage, o64 = _tie_oracle(kind)
    out = dev.out(2, 1, TIE_N)
    dev.call("ntk_dnc_write_allocation_weights", dev.inp(usage), None, out, 2, TIE_N, 1)
    got = out.written()
    close(got, o64, ALLOC_BOUND, "allocation weights with ties (%s)" % kind)
    if kind == "zero":
        assert (got[:, 0, 0] == np.float32(1) - np.float32(1e-6)).all() and got[:, 0, 1:].max() < 2e-6          # slot 1: (1 - 1e-6) 1e-6
    if kind == "lowest_tied":
        assert got[0, 0, 5] > 0.9 and got[0, 0, 1050] < 0.1 and got[1, 0, 1023] > 0.9 and got[1, 0, 1024] < 0.1


# ------------------------------------------------------------------------------------------------------ interface activations
def _selection_params(cfg, dtype):
    """Parameters that make oracle.read_inputs / access_step take their ten linears' outputs straight from the columns of h (the raw
    interface row in the packed order of DncDims): 0 / 1 selection matrices, zero biases.  h @ w is then exact in any precision."""
    I = sum(w for _n, w in cfg.interface)
    p, o = {}, 0
    for name, width in cfg.interface:
        w = np.zeros((I, width), dtype)
        w[np.arange(o, o + width), np.arange(width)] = 1
        p["memory_access/%s/w" % name], p["memory_access/%s/b" % name] = w, np.zeros(width, dtype)
        o += width
    return p, I


FIELDS = ("write_vectors", "erase_vectors", "free_gate", "allocation_gate", "write_gate", "read_mode", "write_content_keys",
          "write_content_strengths", "read_content_keys", "read_content_strengths")       # the order of DncDims' offsets
PASSED_THROUGH = ("write_vectors", "write_content_keys", "write_content_strengths", "read_content_keys", "read_content_strengths")


@functools.lru_cache(maxsize=None)
def _interface_oracle(W, R, Wn):
    B = 3
    cfg = D.AccessConfig(16, W, R, Wn)
    p64, I = _selection_params(cfg, np.float64)
    raw = (3 * np.random.default_rng(W + R + Wn).standard_normal((B, I))).astype(np.float32)
    i64 = D.read_inputs(cfg, p64, f64(raw))
    i32 = D.read_inputs(cfg, _selection_params(cfg, np.float32)[0], raw)
    return raw, I, i64, _bound("interface", 1e-6, [i32[k] for k in FIELDS], [i64[k] for k in FIELDS])


@pytest.mark.parametrize("W,R,Wn", [(1, 1, 1), (20, 4, 2), (24, 4, 2), (64, 4, 4)])
def test_interface_activations(dev, W, R, Wn):
    raw, I, i64, bound = _interface_oracle(W, R, Wn)
    B, N = 3, 16
    graw = Guarded(B, I, I + 5, dev.cuda, before=1, after=1, init=raw, payload=INPUT_NAN)
    act = dev.out(B * I)
    dev.call("ntk_dnc_interface_activations", graw, I + 5, act, B, N, W, R, Wn)
    flat, o = act.written(), 0
    for name in FIELDS:                                   # field f of every batch element is contiguous: [B, width] at B * offset
        ref = i64[name].reshape(B, -1)
        got = flat[B * o:B * (o + ref.shape[1])].reshape(B, -1)
        if name in PASSED_THROUGH:
            assert raw_bytes_equal(got, raw[:, o:o + ref.shape[1]]), name
        close(got, ref, bound, name)
        if name == "read_mode":
            close(got.reshape(B, R, 1 + 2 * Wn).sum(2), np.ones((B, R)), 1e-6, "read modes sum to 1")
        o += ref.shape[1]
    assert o == I


# ------------------------------------------------------------------------------- erase-and-write, read words, the two mixes
@functools.lru_cache(maxsize=None)
def _erase_oracle(N, W):
    B, Wn = 2, 3
    rng = np.random.default_rng(N * 1000 + W)
    mem = (8 * (rng.random((B, N, W)) - 0.5)).astype(np.float32)
    ww = rng.random((B, Wn, N)).astype(np.float32); ww /= ww.sum(2, keepdims=True) + 1
    er, val = rng.random((B, Wn, W)).astype(np.float32), rng.standard_normal((B, Wn, W)).astype(np.float32)
    o64 = D.erase_and_write(f64(mem), f64(ww), f64(er), f64(val))
    return mem, ww, er, val, o64, _bound("erase_and_write", 2e-5, [D.erase_and_write(mem, ww, er, val)], [o64])


@pytest.mark.parametrize("N,W", [(1, 1), (33, 31), (32, 32), (41, 25), (130, 20)])
def test_erase_and_write(dev, N, W):
    mem, ww, er, val, o64, bound = _erase_oracle(N, W)
    out = dev.out(2, N, W)
    dev.call("ntk_dnc_erase_and_write", dev.inp(mem), dev.inp(ww), dev.inp(er), dev.inp(val), out, 2, N, W, 3)
    close(out.written(), o64, bound, "memory")


@functools.lru_cache(maxsize=None)
def _read_words_oracle(W):
    B, R, N = 2, 3, 20
    st = _rand_state(np.random.default_rng(W), B, N, W, R, 1)
    mem = (8 * st.memory).astype(np.float32)
    o64 = f64(st.read_weights) @ f64(mem)
    return st.read_weights, mem, o64, _bound("read_words", 2e-5, [st.read_weights @ mem], [o64])


@pytest.mark.parametrize("W", [1, 127, 128, 129])
def test_read_words(dev, W):
    rw, mem, o64, bound = _read_words_oracle(W)
    out = dev.out(2, 3, W)
    dev.call("ntk_dnc_read_words", dev.inp(rw), dev.inp(mem), out, 2, 20, W, 3)
    close(out.written(), o64, bound, "read words")


#          B, N, W, R, Wn
MIXES = [(2, 260, 20, 3, 2),      # N = 260 > the 256 threads of a write_mix / read_mix block
         (2, 1, 1, 1, 1),         # every dimension at its minimum
         (130, 3, 2, 2, 2)]       # B Wn = 260 gate products > one block of 256: gate_product_kernel's second block


@functools.lru_cache(maxsize=None)
def _mix_oracle(B, N, W, R, Wn):
    rng = np.random.default_rng(B + N)
    st = _rand_state(rng, B, N, W, R, Wn)
    cfg = D.AccessConfig(N, W, R, Wn)
    mode = rng.random((B, R, 1 + 2 * Wn)).astype(np.float32); mode /= mode.sum(2, keepdims=True)
    inp = {"allocation_gate": rng.random((B, Wn)), "write_gate": rng.random((B, Wn)), "write_content_keys": rng.standard_normal((B, Wn, W)),
           "write_content_strengths": 3 * rng.standard_normal((B, Wn)), "read_content_keys": rng.standard_normal((B, R, W)),
           "read_content_strengths": 3 * rng.standard_normal((B, R)), "read_mode": mode}
    inp = {k: v.astype(np.float32) for k, v in inp.items()}
    i64 = {k: f64(v) for k, v in inp.items()}
    w32, w64 = D.write_weights(cfg, inp, st.memory, st.usage), D.write_weights(cfg, i64, f64(st.memory), f64(st.usage))
    assert np.max(np.abs(f64(w32) - w64)) <= 2e-6 / 4, "ill-conditioned allocation inside the write weights: change the seed"
    r32 = D.read_weights(cfg, inp, st.memory, st.read_weights, st.linkage.link)
    r64 = D.read_weights(cfg, i64, f64(st.memory), f64(st.read_weights), f64(st.linkage.link))
    return st, inp, w64, _bound("write_weights", 2e-6, [w32], [w64]), r64, _bound("read_weights", 2e-5, [r32], [r64])


@pytest.mark.parametrize("B,N,W,R,Wn", MIXES)
def test_write_weights_gate_product_and_mix(dev, B, N, W, R, Wn):
    st, inp, w64, bound, _r, _b = _mix_oracle(B, N, W, R, Wn)
    out, ws = dev.out(B, Wn, N), dev.out(2 * B * Wn * N + B * Wn)
    dev.call("ntk_dnc_write_weights", dev.inp(st.memory), dev.inp(st.usage), dev.inp(inp["write_content_keys"]),
             dev.inp(inp["write_content_strengths"]), dev.inp(inp["allocation_gate"]), dev.inp(inp["write_gate"]), out, ws, B, N, W, Wn)
    close(out.written(), w64, bound, "write weights")
    scratch = ws.written()                     # content | allocation | gate product, all of it written
    close(scratch[2 * B * Wn * N:], (f64(inp["allocation_gate"]) * f64(inp["write_gate"])).ravel(), 1e-6, "gate product")


@pytest.mark.parametrize("B,N,W,R,Wn", MIXES)
def test_read_weights_mix(dev, B, N, W, R, Wn):
    st, inp, _w, _b, r64, bound = _mix_oracle(B, N, W, R, Wn)
    out, ws = dev.out(B, R, N), dev.out(B * R * N * (1 + 2 * Wn))
    dev.call("ntk_dnc_read_weights", dev.inp(st.memory), dev.inp(st.read_weights), dev.inp(st.linkage.link), dev.inp(inp["read_content_keys"]),
             dev.inp(inp["read_content_strengths"]), dev.inp(inp["read_mode"]), out, ws, B, N, W, R, Wn)
    close(out.written(), r64, bound, "read weights")
    ws.written()


# ------------------------------------------------------------------------------------------------------- the composed forward
STEP_KEYS = ("memory", "read_weights", "write_weights", "link", "precedence", "usage", "reads")


def _flat_state(st, reads):
    return dict(memory=st.memory, read_weights=st.read_weights, write_weights=st.write_weights, link=st.linkage.link,
                precedence=st.linkage.precedence_weights, usage=st.usage, reads=reads)


@functools.lru_cache(maxsize=None)
def _step_oracle(N, W, R, Wn, steps=3):
    B = 2
    rng = np.random.default_rng(N + W)
    cfg = D.AccessConfig(N, W, R, Wn)
    p32, I = _selection_params(cfg, np.float32)
    p64, _ = _selection_params(cfg, np.float64)
    st0 = _rand_state(rng, B, N, W, R, Wn)
    s32, s64 = st0, D.AccessState(f64(st0.memory), f64(st0.read_weights), f64(st0.write_weights),
                                  D.TemporalLinkageState(f64(st0.linkage.link), f64(st0.linkage.precedence_weights)), f64(st0.usage))
    raws, refs, bounds = [], [], []
    for _t in range(steps):
        raw = (2 * rng.standard_normal((B, I))).astype(np.float32)
        r32, s32, _ = D.access_step(cfg, p32, raw, s32)
        r64, s64, _ = D.access_step(cfg, p64, f64(raw), s64)
        a, b = _flat_state(s32, r32), _flat_state(s64, r64)
        raws.append(raw); refs.append(b)
        bounds.append(_bound("access_step_fwd", 2e-5, [a[k] for k in STEP_KEYS], [b[k] for k in STEP_KEYS]))
        # conditioning (the allocation sort sits inside): the float32 oracle stays within the bound's floor of the float64 one
        assert bounds[-1] <= 4e-5, "ill-conditioned step (3 x float32-vs-float64 oracle = %.3g): change the seed" % bounds[-1]
    return I, st0, raws, refs, bounds


@pytest.mark.parametrize("N,W,R,Wn", [(260, 20, 4, 2), (64, 132, 2, 1)])
def test_access_step_fwd_three_steps(dev, N, W, R, Wn):
    B = 2
    I, st0, raws, refs, bounds = _step_oracle(N, W, R, Wn)
    shapes = dict(memory=(B, N, W), read_weights=(B, R, N), write_weights=(B, Wn, N), link=(B, Wn, N, N), precedence=(B, Wn, N),
                  usage=(B, N), reads=(B, R, W))
    prev = {k: dev.inp(v) for k, v in _flat_state(st0, np.zeros(shapes["reads"], np.float32)).items()}
    wsn = dev.L.ntk_dnc_access_step_workspace_bytes(B, N, W, R, Wn) // 4
    order = ("memory", "read_weights", "write_weights", "link", "precedence", "usage")
    for t, raw in enumerate(raws):
        graw = Guarded(B, I, I + 5, dev.cuda, before=1, after=1, init=raw, payload=INPUT_NAN)
        new, ws = {k: dev.out(*shapes[k]) for k in STEP_KEYS}, dev.out(wsn)
        dev.call("ntk_dnc_access_step_fwd", graw, I + 5, *([prev[k] for k in order] + [new[k] for k in order] + [new["reads"], ws, B, N, W, R, Wn]))
        for k in STEP_KEYS:
            close(new[k].written(), refs[t][k], bounds[t], "step %d %s" % (t, k))
        assert ws.guards_intact() and all(prev[k].guards_intact() for k in order)
        prev = new
    # a previous-state buffer handed in as its own output is refused before anything is launched
    for k in ("memory", "link", "read_weights", "usage"):
        outs = {q: dev.out(*shapes[q]) for q in order}
        outs[k] = prev[k]
        rc = dev.L.ntk_dnc_access_step_fwd(graw.ptr, I + 5, *([prev[q].ptr for q in order] + [outs[q].ptr for q in order]
                                                               + [dev.out(*shapes["reads"]).ptr, ws.ptr, B, N, W, R, Wn, dev.st]))
        assert rc == BAD_PTR and b"ntk_dnc_access_step_fwd" in dev.L.ntk_last_error(), k


# ------------------------------------------------------------------------------------------------------ the one-step backward
@pytest.mark.parametrize("N,W,R,Wn", [(64, 16, 4, 4), (128, 20, 4, 2)])
def test_access_step_bwd_at_its_limits(dev, N, W, R, Wn):
    """ntk_dnc_access_step_bwd against float64 autograd through oracle/dnc_oracle_torch.access_step from a non-degenerate state; the
    rule of test_memory_access_step_gradients_match_autograd: per tensor, error relative to its largest entry (floored at 1e-3 of
    the largest entry of all gradients) at most 3e-3."""
    B = 2
    rng = np.random.default_rng(N + Wn)
    cfg = D.AccessConfig(N, W, R, Wn)
    p64, I = _selection_params(cfg, np.float64)
    IP = (I + 3) // 4 * 4
    st = _rand_state(rng, B, N, W, R, Wn)
    raw = rng.standard_normal((B, I)).astype(np.float32)
    Gr = rng.standard_normal((B, R, W)).astype(np.float32)
    t64 = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True)
    xt = t64(raw)
    leaves = dict(memory=t64(st.memory), read_weights=t64(st.read_weights), link=t64(st.linkage.link),
                  precedence=t64(st.linkage.precedence_weights), usage=t64(st.usage))
    ost = DT.AccessState(leaves["memory"], leaves["read_weights"], torch.tensor(st.write_weights, dtype=torch.float64),
                         DT.TemporalLinkageState(leaves["link"], leaves["precedence"]), leaves["usage"])
    reads, _new = DT.access_step(cfg, {k: torch.tensor(v) for k, v in p64.items()}, xt, ost)
    (reads * torch.tensor(Gr, dtype=torch.float64)).sum().backward()
    ref = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in leaves.items()}
    ref["raw"] = xt.grad.numpy()
    # HIP: the upstream gradients of the new state are zero (in/out buffers), d loss / d read words = Gr
    graw = Guarded(B, I, IP, dev.cuda, before=1, after=1, init=raw, payload=INPUT_NAN)
    g = {k: FlatGuarded(tuple(v.shape), dev.cuda, init=np.zeros(tuple(v.shape), np.float32), payload=GUARD_NAN) for k, v in leaves.items()}
    d_raw = Guarded(B, I, IP, dev.cuda, before=1, after=1)
    ws = dev.out(dev.L.ntk_dnc_access_step_bwd_workspace_bytes(B, N, W, R, Wn) // 4)
    dev.call("ntk_dnc_access_step_bwd", graw, IP, dev.inp(st.memory), dev.inp(st.read_weights), dev.inp(st.write_weights),
             dev.inp(st.linkage.link), dev.inp(st.linkage.precedence_weights), dev.inp(st.usage), dev.inp(Gr), g["memory"],
             g["read_weights"], g["link"], g["precedence"], g["usage"], d_raw, ws, B, N, W, R, Wn)
    got = {k: v.written() for k, v in g.items()}
    got["raw"] = d_raw.logical()
    assert not np.isnan(got["raw"]).any() and ws.guards_intact()
    h = d_raw.buf.view(torch.int32).cpu().numpy()
    assert (h[0] == GUARD_NAN).all() and (h[-1] == GUARD_NAN).all(), "guard rows around d_iface_raw"
    scale = max(float(np.abs(v).max()) for v in ref.values())
    for k in sorted(ref):
        err = np.max(np.abs(got[k] - ref[k])) / max(np.max(np.abs(ref[k])), 1e-3 * scale)
        assert err < 3e-3, (k, err)


# -------------------------------------------------------------------------------------------------------------------- NTM ops
MODES = ("as_coded", "smooth_cosine")


@functools.lru_cache(maxsize=None)
def _sim_oracle(N, Md, H, mode, zeros=False):
    B = 2
    rng = np.random.default_rng(N * 7 + Md * 3 + H)
    mem, keys = rng.standard_normal((B, N, Md)).astype(np.float32), rng.standard_normal((B, H, Md)).astype(np.float32)
    if zeros:
        mem[0, 2, :] = 0; mem[1, :, Md - 1] = 0; mem[0, :, 0] = 0; keys[0, H - 1] = 0; keys[1, 0] = 0
    o64 = O.batched_smooth_cosine_similarity(f64(mem), f64(keys), MODES[mode])
    assert np.isfinite(o64).all()
    bound = _bound("ntm_cosine_similarity", 2e-6, [O.batched_smooth_cosine_similarity(mem, keys, MODES[mode])], [o64], rule=Md > 20)
    return mem, keys, o64, bound


@pytest.mark.parametrize("mode", [0, 1], ids=MODES)
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("Md", [1, 20, 300])
@pytest.mark.parametrize("N", [1, 63, 257])
def test_ntm_cosine_similarity(dev, N, Md, H, mode):
    mem, keys, o64, bound = _sim_oracle(N, Md, H, mode)
    out = dev.out(2, H, N)
    dev.call("ntk_ntm_cosine_similarity", dev.inp(mem), dev.inp(keys), out, 2, N, Md, H, mode)
    close(out.written(), o64, bound, "similarity")


@pytest.mark.parametrize("mode", [0, 1], ids=MODES)
def test_ntm_cosine_similarity_zero_row_column_and_key(dev, mode):
    """An all-zero memory row, two all-zero feature columns and all-zero keys: finite, and the oracle's clamped form (mode 0:
    x / sqrt(max(sum x^2, 1e-12)); mode 1: dot / (|m| |k| + 1e-3))."""
    N, Md, H = 63, 20, 5
    mem, keys, o64, bound = _sim_oracle(N, Md, H, mode, True)
    out = dev.out(2, H, N)
    dev.call("ntk_ntm_cosine_similarity", dev.inp(mem), dev.inp(keys), out, 2, N, Md, H, mode)
    got = out.written()
    assert np.isfinite(got).all()
    close(got, o64, bound, "similarity with zeros")
    assert not got[0, H - 1].any() and not got[1, 0].any()


CONV_CASES = [(N, SS) for N in (1, 2, 3, 255, 256, 257) for SS in sorted({1, 2, 3, 4, 5, N}) if SS <= N]


@functools.lru_cache(maxsize=None)
def _conv_oracle(N, SS):
    B, H = 2, 3
    rng = np.random.default_rng(N * 10 + SS)
    # what the op convolves in the cell: a weighting over the N slots and a softmax over the shift space, each summing to 1 (so
    # that SS = N = 257 taps still add up to a number below 1, which 1e-6 absolute can be asked of)
    w, s = rng.random((B, H, N)), rng.random((B, H, SS))
    w, s = (w / w.sum(2, keepdims=True)).astype(np.float32), (s / s.sum(2, keepdims=True)).astype(np.float32)
    o64 = O.batched_circular_convolution(f64(w), f64(s))
    _bound("ntm_circular_convolution", 1e-6, [O.batched_circular_convolution(w, s)], [o64])
    return w, s, o64


@pytest.mark.parametrize("N,SS", CONV_CASES)
def test_ntm_circular_convolution(dev, N, SS):
    B, H = 2, 3
    w, s, o64 = _conv_oracle(N, SS)
    dw, out = dev.inp(w), dev.out(B, H, N)
    dev.call("ntk_ntm_circular_convolution", dw, dev.inp(s), out, B, H, N, SS)
    close(out.written(), o64, 1e-6, "circular convolution")
    offs = O.shift_offsets(SS)
    assert offs[0] == -((SS + 1) // 2)
    for j in range(SS):                       # a one-hot kernel on tap j is the circular shift by that tap's offset, bit for bit
        hot = np.zeros((B, H, SS), np.float32); hot[..., j] = 1
        out = dev.out(B, H, N)
        dev.call("ntk_ntm_circular_convolution", dw, dev.inp(hot), out, B, H, N, SS)
        assert raw_bytes_equal(out.written(), O.circular_shift(w, offs[j] % N if N > 1 else 0)), (N, SS, j)


# ----------------------------------------------------------------------------------------------------------- without a device
def oracle_side():
    """Every oracle-side computation and conditioning assertion of this file, without a device; returns the largest float32-vs-
    float64 oracle distance per kernel family (the figures of the module docstring)."""
    OWN.clear()
    for c in COS_CASES:
        _cos_oracle(*c)
    for N in (1, 17, 64, 255, 256, 257, 300):
        for Wn in (1, 3):
            _linkage_oracle(N, Wn)
    for N in (1, 255, 256, 257):
        _directional_oracle(N)
    for N in (1, 256, 257):
        _freeness_oracle(N)
    for c in ALLOC_CASES:
        _alloc_oracle(*c)
    for kind in ("two", "three", "zero", "one", "lowest_tied"):
        _tie_oracle(kind)
    for c in ((1, 1, 1), (20, 4, 2), (24, 4, 2), (64, 4, 4)):
        _interface_oracle(*c)
    for c in ((1, 1), (33, 31), (32, 32), (41, 25), (130, 20)):
        _erase_oracle(*c)
    for W in (1, 127, 128, 129):
        _read_words_oracle(W)
    for c in MIXES:
        _mix_oracle(*c)
    for c in ((260, 20, 4, 2), (64, 132, 2, 1)):
        _step_oracle(*c)
    for N in (1, 63, 257):
        for Md in (1, 20, 300):
            for H in (1, 5):
                for mode in (0, 1):
                    _sim_oracle(N, Md, H, mode)
    for mode in (0, 1):
        _sim_oracle(63, 20, 5, mode, True)
    for c in CONV_CASES:
        _conv_oracle(*c)
    return dict(OWN)


if __name__ == "__main__":
    for k, v in sorted(oracle_side().items()):
        print("%-28s %.2g" % (k, v))
