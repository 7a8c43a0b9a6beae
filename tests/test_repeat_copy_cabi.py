"""CPU: the C ABI of the repeat-copy task (ntk_repeat_copy_pack, ntk_masked_sigmoid_xent) is exported, bound and declared, and
refuses null pointers and bad sizes on the host with its name in ntk_last_error (a refused call never reaches the device, so no GPU
is needed); RepeatCopy and RepeatCopyTask refuse bad arguments before they touch a device."""
import ctypes
import os
import re

import pytest

ONE = ctypes.c_void_p(16)                       # non-null, aligned, never dereferenced: the checks fire first


@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


def pack(L, bits=ONE, lengths=ONE, repeats=ONE, X=ONE, target=ONE, mask=ONE, B=2, S=9, num_bits=4, ldx=8, min_length=1, max_length=2,
         min_repeats=1, max_repeats=2, norm_max=10.0):
    return L.ntk_repeat_copy_pack(bits, lengths, repeats, X, target, mask, B, S, num_bits, ldx, min_length, max_length, min_repeats,
                                  max_repeats, norm_max, None)


def xent(L, logits=ONE, target=ONE, mask=ONE, loss=ONE, loss_batch=ONE, dlogits=None, score=None, B=2, S=9, O=5, time_average=0,
         bits=0):
    return L.ntk_masked_sigmoid_xent(logits, target, mask, loss, loss_batch, dlogits, score, B, S, O, time_average, bits, None)


def test_symbols_are_exported_bound_and_declared(L):
    from ntmtrack import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")).read()
    for name, nargs in (("ntk_repeat_copy_pack", 16), ("ntk_masked_sigmoid_xent", 13)):
        assert hasattr(L, name), "libntmtrack_hip.so does not export %s" % name
        assert name in _lib.exported_symbols()
        assert len(getattr(L, name).argtypes) == nargs
        assert re.search(r"^int %s\(" % name, hdr, re.M), "%s is not declared in include/ntmtrack.h" % name


@pytest.mark.parametrize("arg", ["bits", "lengths", "repeats", "X", "target", "mask"])
def test_pack_refuses_null_pointers(L, arg):
    assert pack(L, **{arg: None}) == -2
    assert b"ntk_repeat_copy_pack" in L.ntk_last_error()


@pytest.mark.parametrize("kw,named", [({"B": 0}, b"B=0"), ({"num_bits": 0}, b"num_bits=0"), ({"ldx": 4}, b"ldx=4"),
                                      ({"num_bits": 3, "ldx": 6}, b"ldx=6"), ({"ldx": 10}, b"ldx=10"),
                                      ({"S": 4}, b"S=4"), ({"S": 8, "min_length": 2, "min_repeats": 2}, b"S=8"),
                                      ({"min_length": 3}, b"[3, 2]"), ({"min_repeats": 3}, b"[3, 2]"), ({"min_length": 0}, b"[0, 2]")])
def test_pack_refuses_bad_sizes_and_names_the_value(L, kw, named):
    assert pack(L, **kw) == -1
    assert named in L.ntk_last_error() and b"ntk_repeat_copy_pack" in L.ntk_last_error()


def test_pack_takes_the_smallest_step_count_of_its_ranges_as_far_as_the_host_can_tell(L):
    """S = min_length (min_repeats + 1) + 3 passes every host check: with a misaligned X the NEXT clause refuses."""
    assert pack(L, S=5, X=ctypes.c_void_p(20)) == -2
    assert b"aligned" in L.ntk_last_error()


@pytest.mark.parametrize("arg", ["logits", "target", "mask", "loss", "loss_batch"])
def test_xent_refuses_null_pointers(L, arg):
    assert xent(L, **{arg: None}) == -2
    assert b"ntk_masked_sigmoid_xent" in L.ntk_last_error()


@pytest.mark.parametrize("kw,named", [({"B": 0}, b"B=0"), ({"S": 0}, b"S=0"), ({"O": 0}, b"O=0"), ({"S": 1 << 20, "O": 1 << 11}, b"O=2048")])
def test_xent_refuses_bad_sizes_and_names_the_value(L, kw, named):
    assert xent(L, **kw) == -1
    assert named in L.ntk_last_error() and b"ntk_masked_sigmoid_xent" in L.ntk_last_error()


@pytest.mark.parametrize("kw", [{"min_length": 3, "max_length": 2}, {"min_repeats": 3, "max_repeats": 2}, {"num_bits": 0},
                                {"batch_size": 0}, {"min_length": 0}, {"norm_max": 0}])
def test_repeat_copy_refuses_bad_arguments(kw):
    from ntmtrack import _lib
    from ntmtrack.repeat_copy import RepeatCopy
    with pytest.raises(_lib.NtkError, match="RepeatCopy"):
        RepeatCopy(**kw)


def test_task_refuses_what_the_dnc_bptt_launcher_refuses_before_anything_is_launched():
    """num_bits = 16 is 17 outputs; ntk_dnc_seq_bwd takes at most 16.  The launcher's own message comes back."""
    from ntmtrack import _lib
    from ntmtrack.repeat_copy import RepeatCopy, RepeatCopyTask
    with pytest.raises(_lib.NtkError, match="ntk_dnc_seq_bwd.*output=17"):
        RepeatCopyTask(RepeatCopy(num_bits=16, batch_size=2))
    with pytest.raises(_lib.NtkError, match="ntk_dnc_seq_bwd.*num_writes=5"):
        RepeatCopyTask(RepeatCopy(num_bits=4, batch_size=2), num_writes=5)
    with pytest.raises(_lib.NtkError, match="mem_size=16"):                   # the NTM sequence kernels take 64 slots or more
        RepeatCopyTask(RepeatCopy(num_bits=4, batch_size=2), core="ntm")
    with pytest.raises(_lib.NtkError, match="core="):
        RepeatCopyTask(RepeatCopy(num_bits=4, batch_size=2), core="lstm")
