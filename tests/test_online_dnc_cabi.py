"""CPU: the C ABI and the host bookkeeping of the online DNC tracker.  ntk_dnc_state_keep is exported and bound and refuses
every invalid argument on the host, before anything is launched (no GPU is needed: a refused call never reaches the device);
the new public names exist; a serving state converts to the logical state shapes for a word size that needs padding and for
one that does not."""
import ctypes

import pytest
import torch

ONE = ctypes.c_void_p(16)                       # non-null, aligned, never dereferenced: the checks fire first
BAD_SHAPE, BAD_PTR = -1, -2


@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


def keep(L, mask=ONE, keep_where=0, B=2, ntensors=2, src=ONE, dst=ONE, rows=(8, 20)):
    arr = None if rows is None else (ctypes.c_longlong * len(rows))(*rows)
    return L.ntk_dnc_state_keep(mask, keep_where, B, ntensors, src, dst, arr, None)


def test_state_keep_is_exported_and_bound(L):
    from ntmtrack import _lib
    assert hasattr(L, "ntk_dnc_state_keep"), "libntmtrack_hip.so does not export ntk_dnc_state_keep"
    assert "ntk_dnc_state_keep" in _lib.exported_symbols()
    assert L.ntk_dnc_state_keep.argtypes is not None and len(L.ntk_dnc_state_keep.argtypes) == 8


@pytest.mark.parametrize("arg", ["mask", "src", "dst", "rows"])
def test_state_keep_refuses_null_pointers(L, arg):
    assert keep(L, **{arg: None}) == BAD_PTR


@pytest.mark.parametrize("kw,named", [({"B": 0}, b"B=0"), ({"B": -2}, b"B=-2"), ({"B": 65536}, b"B=65536"),
                                      ({"ntensors": 0}, b"ntensors=0"), ({"ntensors": -1}, b"ntensors=-1"),
                                      ({"ntensors": 17, "rows": (4,) * 17}, b"ntensors=17"),
                                      ({"rows": (8, -4)}, b"row_floats[1]=-4"), ({"rows": (-1, 4)}, b"row_floats[0]=-1")])
def test_state_keep_refuses_bad_shapes_and_names_the_value(L, kw, named):
    assert keep(L, **kw) == BAD_SHAPE
    assert named in L.ntk_last_error()


def test_the_table_limit_of_the_header_is_sixteen():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")).read()
    assert re.search(r"#define NTK_STATE_KEEP_MAX_TENSORS\s+16\b", hdr)
    assert "int ntk_dnc_state_keep(" in hdr


def test_the_public_names_exist():
    from ntmtrack import dnc, online
    for name in ("BatchDNCTracker", "DNCTracker", "state_keep"):
        assert hasattr(online, name), name
    assert issubclass(online.BatchDNCTracker, online.BatchNTMTracker)
    for m in ("track", "track_clip", "reset", "check", "from_tracker"):
        assert callable(getattr(online.BatchDNCTracker, m)), m
    assert callable(online.DNCTracker.track)
    assert callable(dnc.DNC.serving_state) and callable(dnc.DNC.serve_projected)


def _core(word_size, Wn=1):
    from ntmtrack.dnc import DNC
    return DNC({"memory_size": 24, "word_size": word_size, "num_reads": 2, "num_writes": Wn}, {"hidden_size": 12}, 2, device="cpu")


def _leaves(st):
    a = st.access_state
    return {"reads": st.access_output, "memory": a.memory, "rw": a.read_weights, "ww": a.write_weights, "link": a.linkage.link,
            "prec": a.linkage.precedence_weights, "usage": a.usage, "h": st.controller_state.hidden, "c": st.controller_state.cell}


@pytest.mark.parametrize("word_size,Wn", [(5, 1), (8, 1), (6, 3)], ids=["w5_padded", "w8_exact", "w6_three_writes"])
def test_serving_state_layout(word_size, Wn):
    core = _core(word_size, Wn)
    B, N, R, hid, Wp = 3, 24, 2, 12, (word_size + 3) // 4 * 4
    s = core.serving_state(B)
    # the buffers as the forward launchers take them: padded words, hc = [hidden, cell], zero, contiguous
    want = {"mem": (B, N, Wp), "link": (B, Wn, N, N), "usage": (B, N), "rw": (B, R, N), "ww": (B, Wn, N), "prec": (B, Wn, N),
            "reads": (B, R, Wp), "hc": (B, 2 * hid)}
    assert s.NAMES == tuple(want)
    for (name, shape), t, n in zip(want.items(), s.tensors(), s.row_floats()):
        assert tuple(t.shape) == shape and t.is_contiguous() and t.dtype == torch.float32 and not t.any(), name
        assert n == t[0].numel()
    # every row of the padded layout is a whole number of 16-byte vectors when memory_size is a multiple of 4 (the kernels need that)
    assert all(n % 4 == 0 for n in s.row_floats())
    # to_state: the logical shapes of initial_state
    got, ref = _leaves(s.to_state()), _leaves(core.initial_state(B))
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].is_contiguous() and not got[k].any(), k


@pytest.mark.parametrize("word_size", [5, 8])
def test_serving_state_load_round_trip_and_scatter(word_size):
    core = _core(word_size)
    g = torch.Generator().manual_seed(word_size)

    def rnd(x):                                                        # the same (nested) state tuple with random leaves
        if isinstance(x, tuple):
            return type(x)(*[rnd(y) for y in x])
        return torch.rand(x.shape, generator=g) + 0.5                  # no zeros: a lost element shows
    full = rnd(core.initial_state(3))
    s = core.serving_state(3).load(full)
    for k, v in _leaves(s.to_state()).items():
        assert torch.equal(v, _leaves(full)[k]), k
    if word_size == 5:
        assert not s.mem[..., 5:].any() and not s.reads[..., 5:].any() and s.mem[..., :5].all()
    # hc is hidden then cell
    assert torch.equal(s.hc[:, :12], full.controller_state.hidden) and torch.equal(s.hc[:, 12:], full.controller_state.cell)
    # scatter two sequences into slots 2 and 0 of a state whose padding was dirtied: slot 1 untouched, the padding of 2 and 0 zero
    two = rnd(core.initial_state(2))
    before = [t.clone() for t in s.tensors()]
    s.mem[..., word_size:] = 7.0
    before[0] = s.mem.clone()
    s.load(two, rows=[2, 0])
    got, want, old = _leaves(s.to_state()), _leaves(two), _leaves(full)
    for k in got:
        assert torch.equal(got[k][2], want[k][0]) and torch.equal(got[k][0], want[k][1]) and torch.equal(got[k][1], old[k][1]), k
    for t, b in zip(s.tensors(), before):
        assert torch.equal(t[1], b[1])
    if word_size == 5:
        assert not s.mem[[2, 0], :, 5:].any() and (s.mem[1, :, 5:] == 7.0).all()
    from ntmtrack._lib import NtkError
    with pytest.raises(NtkError):
        s.load(two)                                                    # batch 2 into a state of 3
