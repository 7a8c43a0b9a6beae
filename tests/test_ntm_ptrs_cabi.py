"""CPU: the pointer checks of the four NTM sequence launchers (ntk_ntm_seq_fwd, ntk_ntm_seq_bwd, ntk_ntm_seq_fwd_deep,
ntk_ntm_seq_bwd_deep) in their plain, *_sim and step forms.

Every entry is called with fake pointers that are never dereferenced: a call that passes every host-side check reaches the
device calls, which fail without a device (NTK_ERR_HIP); a null required pointer, a misaligned pointer of the launcher's 16-byte
set or a broken pairing rule is refused before them (NTK_ERR_BAD_PTR); a bad leading dimension is refused before any pointer is
looked at (NTK_ERR_BAD_SHAPE).  With a device present an accepted call would launch against the fake pointers, so the file runs
only where there is none (as tests/test_ntm_shapes_cabi.py)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: runs only where no device is visible")

NTK_ERR_BAD_SHAPE, NTK_ERR_BAD_PTR, NTK_ERR_HIP = -1, -2, -4
GOOD, ODD = 1 << 20, (1 << 20) + 4                               # 16-byte aligned; addr % 16 == 4
TRACKER = (128, 20, 4, 1, 200, 1, 2)                             # N, Md, R, Wh, hid, shift_range, O
BATCH, STEPS, DIN = 2, 3, 10
LDKT, LDHT = 280, 200                                            # align4(R Md + hid), align4(hid)

FWD_RECORDS = ["st_z", "st_gates", "st_c", "st_h", "st_u", "st_wc", "st_wv", "st_w", "st_M", "st_read"]
FWD = dict(
    names=["xproj", "Wr", "Wa", "M0", "w0", "read0", "cs0", "logits", "outputs", "M_out", "w_out", "read_out", "cs_out"] + FWD_RECORDS,
    nullable=["outputs"] + FWD_RECORDS, aligned=["xproj", "Wr", "Wa", "st_gates"])
BWD = dict(
    names=["WrT", "WaT", "M0", "w0", "cs0", "st_gates", "st_c", "st_u", "st_wc", "st_wv", "st_w", "st_M", "dlogits",
           "dM_fin", "dw_fin", "dread_fin", "dcs_fin", "dgates", "du", "dM0", "dw0", "dread0", "dcs0"],
    nullable=["dM_fin", "dw_fin", "dread_fin", "dcs_fin"], aligned=["WrT", "WaT", "st_gates", "dgates"])
DEEP_RECORDS = ["st_xtop", "st_buf0", "st_bufk", "st_lgates", "st_lc"]
FWD_DEEP = dict(
    names=["X", "xproj", "Wf", "Wa", "M0", "w0", "read0", "cs0", "logits", "outputs", "M_out", "w_out", "read_out", "cs_out"] +
    FWD_RECORDS + DEEP_RECORDS,
    nullable=["outputs"] + FWD_RECORDS + DEEP_RECORDS, aligned=["xproj", "Wf", "Wa", "st_gates", "st_lgates"])
BWD_DEEP = dict(
    names=["Wb", "WaT", "M0", "w0", "cs0", "st_gates", "st_c", "st_u", "st_wc", "st_wv", "st_w", "st_M", "st_lgates", "st_lc",
           "dlogits", "dM_fin", "dw_fin", "dread_fin", "dcs_fin", "dgates", "dpre", "du", "dM0", "dw0", "dread0", "dcs0"],
    nullable=["dM_fin", "dw_fin", "dread_fin", "dcs_fin"], aligned=["Wb", "WaT", "st_gates", "st_lgates", "dgates"])


def _lib():
    from ntmtrack import _lib
    return _lib.lib()


def _p(ptrs, names):
    return [None if ptrs[n] is None else ctypes.c_void_p(ptrs[n]) for n in names]


def _lead(form, sim, layers=None):
    """The integer arguments in front of the pointers: B, [S], the dims, [L], write_first, [similarity]."""
    lead = [BATCH] + ([] if form == "step" else [STEPS]) + list(TRACKER) + ([] if layers is None else [layers]) + [0]
    return lead + ([] if sim is None else [sim])


def call_fwd(L, form, sim, ptrs, **_):
    fn = getattr(L, "ntk_ntm_%s_fwd%s" % ("step" if form == "step" else "seq", "" if sim is None else "_sim"))
    return fn(*_lead(form, sim), *_p(ptrs, FWD["names"]), None)


def call_bwd(L, form, sim, ptrs, ldkT=LDKT, ldhT=LDHT, **_):
    fn = getattr(L, "ntk_ntm_%s_bwd%s" % ("step" if form == "step" else "seq", "" if sim is None else "_sim"))
    p = _p(ptrs, BWD["names"])
    return fn(*_lead(form, sim), p[0], ldkT, p[1], ldhT, *p[2:], None)


def call_fwd_deep(L, form, sim, ptrs, layers=2, **_):
    fn = getattr(L, "ntk_ntm_seq_fwd_deep" + ("" if sim is None else "_sim"))
    return fn(*_lead(form, sim, layers), DIN, *_p(ptrs, FWD_DEEP["names"]), None)


def call_bwd_deep(L, form, sim, ptrs, layers=2, ldhT=LDHT, **_):
    fn = getattr(L, "ntk_ntm_seq_bwd_deep" + ("" if sim is None else "_sim"))
    p = _p(ptrs, BWD_DEEP["names"])
    return fn(*_lead(form, sim, layers), p[0], p[1], ldhT, *p[2:], None)


# (launcher, spec, call, layers): the plain entry has no similarity argument (None), the *_sim entries take both modes; the
# single-layer launchers have step forms too
SINGLE_FORMS = [("seq", None), ("seq", 0), ("seq", 1), ("step", None), ("step", 0), ("step", 1)]
DEEP_FORMS = [("seq", None), ("seq", 0), ("seq", 1)]
CASES = [("fwd", FWD, call_fwd, None, f) for f in SINGLE_FORMS] + [("bwd", BWD, call_bwd, None, f) for f in SINGLE_FORMS] + \
    [("fwd_deep", FWD_DEEP, call_fwd_deep, layers, f) for layers in (2, 3) for f in DEEP_FORMS] + \
    [("bwd_deep", BWD_DEEP, call_bwd_deep, layers, f) for layers in (2, 3) for f in DEEP_FORMS]
IDS = ["%s-%s-%s%s" % (c[0], c[4][0], "plain" if c[4][1] is None else "sim%d" % c[4][1], "" if c[3] is None else "-L%d" % c[3]) for c in CASES]


def _all_set(spec):
    return {n: GOOD for n in spec["names"]}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pointer_checks(case):
    name, spec, call, layers, (form, sim) = case
    L = _lib()
    kw = {} if layers is None else {"layers": layers}
    run = lambda ptrs: call(L, form, sim, ptrs, **kw)
    bad = []

    def expect(rc, want, what, word=None):
        msg = L.ntk_last_error() or b""
        if rc != want:
            bad.append("%s: returned %d, expected %d (%s)" % (what, rc, want, msg.decode()))
        elif word is not None and word not in msg:
            bad.append("%s: %r not in the message %r" % (what, word, msg))

    expect(run(_all_set(spec)), NTK_ERR_HIP, "every pointer set")
    forward = "st_z" in spec["names"]
    for n in spec["names"]:
        ptrs = _all_set(spec)
        ptrs[n] = None
        if n in ("st_gates", "st_c") and forward:
            expect(run(ptrs), NTK_ERR_BAD_PTR, "%s null without its partner" % n)      # st_gates and st_c go together
            ptrs["st_gates"] = ptrs["st_c"] = None
            expect(run(ptrs), NTK_ERR_HIP, "st_gates and st_c both null")
        elif n == "X":
            expect(run(ptrs), NTK_ERR_BAD_PTR, "st_buf0 without X")                       # the st_buf0 record needs X
            ptrs["st_buf0"] = None
            expect(run(ptrs), NTK_ERR_HIP, "X and st_buf0 both null")
        elif n in spec["nullable"]:
            expect(run(ptrs), NTK_ERR_HIP, "nullable %s null" % n)
        else:
            expect(run(ptrs), NTK_ERR_BAD_PTR, "required %s null" % n)
    for n in spec["names"]:
        ptrs = _all_set(spec)
        ptrs[n] = ODD
        if n in spec["aligned"]:
            expect(run(ptrs), NTK_ERR_BAD_PTR, "%s at an address %% 16 == 4" % n, b"aligned")
        else:
            expect(run(ptrs), NTK_ERR_HIP, "%s (outside the 16-byte set) at an address %% 16 == 4" % n)
    # every record and every nullable pointer null at once
    ptrs = _all_set(spec)
    for n in spec["nullable"]:
        ptrs[n] = None
    expect(run(ptrs), NTK_ERR_HIP, "all nullable pointers null")
    assert not bad, "%s %s sim=%s:\n  %s" % (name, form, sim, "\n  ".join(bad))


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("bwd", "bwd_deep")],
                         ids=[i for c, i in zip(CASES, IDS) if c[0] in ("bwd", "bwd_deep")])
def test_leading_dimensions_are_refused_before_the_pointers(case):
    """ldkT / ldhT too small or not a multiple of 4: NTK_ERR_BAD_SHAPE with every pointer null."""
    name, spec, call, layers, (form, sim) = case
    L = _lib()
    kw = {} if layers is None else {"layers": layers}
    null = {n: None for n in spec["names"]}
    lds = [{"ldhT": 196}, {"ldhT": 202}] + ([{"ldkT": 276}, {"ldkT": 282}] if name == "bwd" else [])
    for ld in lds:
        assert call(L, form, sim, null, **kw, **ld) == NTK_ERR_BAD_SHAPE, (name, form, sim, ld, L.ntk_last_error())
        assert call(L, form, sim, _all_set(spec), **kw, **ld) == NTK_ERR_BAD_SHAPE, (name, form, sim, ld)
    # good leading dimensions and null pointers: now the pointers are looked at
    assert call(L, form, sim, null, **kw) == NTK_ERR_BAD_PTR
    # wider valid ones are taken
    wide = {"ldhT": 204} if name == "bwd_deep" else {"ldkT": 284, "ldhT": 204}
    assert call(L, form, sim, _all_set(spec), **kw, **wide) == NTK_ERR_HIP, (name, form, sim, L.ntk_last_error())


def test_refusals_come_in_order():
    """similarity, then shape and plan, then pointers: an unknown similarity mode is refused (NTK_ERR_UNSUPPORTED) with a bad shape
    and null pointers, a bad shape with null pointers."""
    L = _lib()
    for spec, call, kw in ((FWD, call_fwd, {}), (BWD, call_bwd, {}), (FWD_DEEP, call_fwd_deep, {"layers": 2}),
                           (BWD_DEEP, call_bwd_deep, {"layers": 2})):
        null = {n: None for n in spec["names"]}
        assert call(L, "seq", 7, null, **kw) == -3 and b"similarity=7" in L.ntk_last_error()
        assert call(L, "seq", 0, null, **kw) == NTK_ERR_BAD_PTR and b"null pointer" in L.ntk_last_error()
