"""Shared pieces of the small-kernel tests (test_gemm_gpu.py, test_small_kernels_gpu.py, test_modules_gpu.py,
test_module_shapes_gpu.py, test_image_kernels_gpu.py): NaN-guarded device buffers and the float64 restatements that more than one
file compares against."""
import ctypes

import numpy as np
import torch


def vptr(t):
    """Device pointer of a tensor's first element; unlike _lib.ptr it takes strided views (padded matrices)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


#: quiet NaNs with distinct payloads: operands' surroundings carry INPUT_NAN, output buffers GUARD_NAN.  A NaN that a kernel
#: computes from an operand's guard and stores over an output guard is then still seen (its bits are not GUARD_NAN's).
INPUT_NAN = 0x7FC00A0A
GUARD_NAN = 0x7FC05EED


def nan_tensor(shape, device, payload=GUARD_NAN):
    shape = shape if isinstance(shape, tuple) else (shape,)
    return torch.full(shape, payload, device=device, dtype=torch.int32).view(torch.float32)


def still_guard(t, payload=GUARD_NAN):
    """Every word of t still holds the prefilled NaN, bit for bit."""
    return bool((t.contiguous().view(torch.int32) == payload).all())


def to_dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


class Guarded(object):
    """A [rows, cols] fp32 matrix living inside a larger NaN-filled device buffer: leading dimension ld >= cols, `before` /
    `after` whole guard rows in front of and behind it.  `view` is the logical matrix, `ptr` its first element."""

    def __init__(self, rows, cols, ld, device, before=0, after=0, init=None, payload=GUARD_NAN):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.before, self.payload = rows, cols, ld, before, payload
        self.buf = nan_tensor((before + rows + after, ld), device, payload)
        self.view = self.buf[before:before + rows, :cols]
        if init is not None:
            self.view.copy_(to_dev(init, device))
        self.ptr = vptr(self.view)

    def logical(self):
        return self.view.cpu().numpy()

    def guards_intact(self):
        """Every element outside the logical matrix still holds the prefilled NaN, bit for bit."""
        h = self.buf.view(torch.int32).cpu().numpy().copy()
        h[self.before:self.before + self.rows, :self.cols] = self.payload
        return bool((h == self.payload).all())


class FlatGuarded(object):
    """A contiguous fp32 array of `shape` inside a NaN-filled device buffer, `pad` words (a multiple of 4: the array stays 16-byte
    aligned) in front of and behind it.  An output starts as GUARD_NAN throughout; an operand (init given) carries `payload` only
    around it -- INPUT_NAN, so that a read past its end turns the result into a NaN that is not the guard's."""

    def __init__(self, shape, device, init=None, payload=None, pad=64):
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
        self.payload = payload if payload is not None else (GUARD_NAN if init is None else INPUT_NAN)
        self.n, self.pad = int(np.prod(shape)), pad
        self.buf = nan_tensor(self.n + 2 * pad, device, self.payload)
        self.view = self.buf[pad:pad + self.n].view(shape)
        if init is not None:
            self.view.copy_(to_dev(np.array(np.broadcast_to(init, shape), np.float32), device))
        self.ptr = vptr(self.view)

    def numpy(self):
        return self.view.cpu().numpy()

    def guards_intact(self):
        return still_guard(self.buf[:self.pad], self.payload) and still_guard(self.buf[self.pad + self.n:], self.payload)

    def written(self):
        """The array on the host, after asserting that every element was written with a number and no guard word was touched."""
        a = self.numpy()
        assert not np.isnan(a).any(), "%d of %d output elements are NaN" % (int(np.isnan(a).sum()), a.size)
        assert self.guards_intact(), "guard words around the output were overwritten"
        return a


def raw_bytes_equal(a, b):
    """Bit-for-bit equality of two arrays of one shape and type (-0.0 differs from 0.0, NaNs compare by payload)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def resize_ref(img, OH, OW):
    """float64 restatement of resize_bilinear_kernel's contract (tf.image.resize_images, BILINEAR, TF-1 defaults): src = dst *
    (in / out), neighbours floor(src) and min(floor(src) + 1, in - 1)."""
    img = np.asarray(img, np.float64)
    H, W, C = img.shape
    ys = np.arange(OH) * (H / OH); xs = np.arange(OW) * (W / OW)
    y0 = np.floor(ys).astype(int); x0 = np.floor(xs).astype(int)
    y1 = np.minimum(y0 + 1, H - 1); x1 = np.minimum(x0 + 1, W - 1)
    fy = (ys - y0)[:, None, None]; fx = (xs - x0)[None, :, None]
    top = img[y0][:, x0] + (img[y0][:, x1] - img[y0][:, x0]) * fx
    bot = img[y1][:, x0] + (img[y1][:, x1] - img[y1][:, x0]) * fx
    return top + (bot - top) * fy


def lstm_pointwise64(pre, c_prev, forget_bias=0.0, dh=None, dc=None):
    """float64 autograd restatement of BasicLSTMCell's pointwise part (ntm_cell.py:45-50): pre [B, 4 hid] in TF's block order
    i | j | f | o; c' = c sigmoid(f + forget_bias) + sigmoid(i) tanh(j); h' = tanh(c') sigmoid(o).
    Returns (c', h', act [B, 4 hid]) and, when dh or dc is given, also (d pre, d c_prev) of sum(h' dh) + sum(c' dc)."""
    hid = c_prev.shape[1]
    p64 = torch.tensor(pre, dtype=torch.float64, requires_grad=True)
    c64 = torch.tensor(c_prev, dtype=torch.float64, requires_grad=True)
    i, j, f, o = p64.split(hid, dim=1)
    gi, gj, gf, go = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + forget_bias), torch.sigmoid(o)
    cr = c64 * gf + gi * gj
    hr = torch.tanh(cr) * go
    act = torch.cat([gi, gj, gf, go], dim=1)
    fwd = (cr.detach().numpy(), hr.detach().numpy(), act.detach().numpy())
    if dh is None and dc is None:
        return fwd
    obj = 0.0
    if dh is not None:
        obj = obj + (hr * torch.tensor(dh, dtype=torch.float64)).sum()
    if dc is not None:
        obj = obj + (cr * torch.tensor(dc, dtype=torch.float64)).sum()
    obj.backward()
    return fwd + (p64.grad.numpy(), c64.grad.numpy())
