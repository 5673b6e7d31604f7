"""Batched engine: thin, typed wrapper over the C ABI (one PairingEngine == one zkp_ctx == one GPU).

Array conventions (numpy uint64 or torch int64/uint64-viewed tensors, C-contiguous):
  g1 (n,12)  g2 (n,24)  inf (n,) uint8  fp12/Gt (n,72)  scalars (n,4)
Host numpy arrays go through the host-pointer entry points (copy in / copy out); torch tensors
that live on the engine's GPU go through the *_dev entry points and never leave HBM."""
import ctypes

import numpy as np

from . import _lib

KERNEL_AUTO, KERNEL_THREAD, KERNEL_COOP = 0, 1, 2


def _np(a, cols, dtype=np.uint64):
    a = np.ascontiguousarray(a, dtype=dtype)
    if cols is not None:
        a = a.reshape(-1, cols)
    return a


def _flags(inf, n, name):
    """optional per-point infinity flags: n bytes"""
    if inf is None:
        return None
    a = np.ascontiguousarray(inf, dtype=np.uint8).reshape(-1)
    if a.size != n:
        raise ValueError("%s: %d flags for %d points" % (name, a.size, n))
    return a


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class PairingEngine:
    def __init__(self, device=0, kernel=None, validate=False):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self._lib.zkp_init(int(device), ctypes.byref(h))
        if rc != 0:
            raise _lib.ZkpError(rc, "zkp_init(device=%d)" % device)
        self._h = h
        self.device = int(device)
        if validate:
            self._chk(self._lib.zkp_set_validate(self._h, 1))
        if kernel is not None:
            self.set_kernel(kernel)

    # ------------------------------------------------------------------ plumbing
    def _chk(self, rc):
        if rc != 0:
            raise _lib.ZkpError(rc, self._lib.zkp_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.zkp_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_kernel(self, kind):
        kind = {"auto": 0, "thread": 1, "coop": 2}.get(kind, kind)
        self._chk(self._lib.zkp_set_kernel(self._h, int(kind)))

    def set_validate(self, on):
        self._chk(self._lib.zkp_set_validate(self._h, 1 if on else 0))

    def take_validation_status(self):
        """validation mode on the device-tensor entry points: True if any such call since the last query saw a field
        element >= p (synchronises the current torch stream; clears the word)"""
        bad = ctypes.c_int(0)
        self._chk(self._lib.zkp_take_validation_status_dev(self._h, self._stream(), ctypes.byref(bad)))
        return bool(bad.value)

    def device_info(self):
        cus, clk = ctypes.c_int(), ctypes.c_int()
        name = ctypes.create_string_buffer(64)
        self._chk(self._lib.zkp_device_info(self._h, ctypes.byref(cus), ctypes.byref(clk), name, 64))
        return {"cus": cus.value, "clock_khz": clk.value, "arch": name.value.decode()}

    @staticmethod
    def gt_identity():
        p = _lib.load().zkp_gt_identity()
        return np.array([p[i] for i in range(72)], dtype=np.uint64)

    # ------------------------------------------------------------------ host-array API
    @staticmethod
    def host_array(shape, dtype=np.uint64):
        """numpy array in page-locked host memory (zkp_host_alloc): the host-pointer entry points copy from / into such an
        array by DMA, overlapped with the kernels; a pageable array works too, its copies block the calling thread.  The
        memory is released when the array (and every view of it) is gone."""
        import weakref
        lib = _lib.load()
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        st = lib.zkp_host_alloc(max(nbytes, 1), ctypes.byref(p))
        if st != 0:
            raise _lib.ZkpError(st, "zkp_host_alloc(%d bytes)" % nbytes)
        buf = (ctypes.c_ubyte * max(nbytes, 1)).from_address(p.value)
        weakref.finalize(buf, lib.zkp_host_free, ctypes.c_void_p(p.value))
        return np.frombuffer(buf, dtype=dtype, count=nbytes // np.dtype(dtype).itemsize).reshape(shape)

    def pairing(self, g1, g2, inf1=None, inf2=None, out=None):
        """out[i] = pairing(g1[i], g2[i])  -> (n,72) canonical Gt (into `out` when given, e.g. a host_array)"""
        if _is_torch(g1):
            if out is not None and not _is_torch(out):
                raise ValueError("out must be a tensor on the engine's GPU when the inputs are")
            return self._pairing_t(g1, g2, inf1, inf2, out)
        g1, g2 = _np(g1, 12), _np(g2, 24)
        n = g1.shape[0]
        if g2.shape[0] != n:
            raise ValueError("g1 and g2 hold different numbers of points")
        i1, i2 = _flags(inf1, n, "inf1"), _flags(inf2, n, "inf2")
        if out is None:
            out = np.empty((n, 72), dtype=np.uint64)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.uint64 and out.shape == (n, 72) and out.flags["C_CONTIGUOUS"]):
            raise ValueError("out must be a C-contiguous (n, 72) uint64 array")
        self._chk(self._lib.zkp_pairing_batch(self._h, _ptr(g1), _ptr(g2), _ptr(i1), _ptr(i2), n, _ptr(out)))
        return out

    def multi_miller_loop(self, g1, g2, k, inf1=None, inf2=None):
        """groups of k consecutive pairs -> (n_checks,72) MillerLoopResult"""
        if _is_torch(g1):
            return self._miller_t(g1, g2, k, inf1, inf2)
        g1, g2 = _np(g1, 12), _np(g2, 24)
        n = g1.shape[0]
        if g2.shape[0] != n or k <= 0 or n % k:
            raise ValueError("g1 / g2 sizes do not match or are not a multiple of k")
        i1, i2 = _flags(inf1, n, "inf1"), _flags(inf2, n, "inf2")
        out = np.empty((n // k, 72), dtype=np.uint64)
        self._chk(self._lib.zkp_multi_miller_loop_batch(self._h, _ptr(g1), _ptr(g2), _ptr(i1), _ptr(i2), n // k, k, _ptr(out)))
        return out

    def final_exponentiation(self, f):
        if _is_torch(f):
            return self._fexp_t(f)
        f = _np(f, 72)
        out = np.empty_like(f)
        self._chk(self._lib.zkp_final_exponentiation_batch(self._h, _ptr(f), f.shape[0], _ptr(out)))
        return out

    def pairing_check(self, g1, g2, k, inf1=None, inf2=None):
        """-> (ok bytes (n_checks,), all_ok bool): prod_j e(g1[c*k+j], g2[c*k+j]) == Gt::identity()"""
        if _is_torch(g1):
            return self._check_t(g1, g2, k, inf1, inf2)
        g1, g2 = _np(g1, 12), _np(g2, 24)
        n = g1.shape[0]
        if g2.shape[0] != n or k <= 0 or n % k:
            raise ValueError("g1 / g2 sizes do not match or are not a multiple of k")
        i1, i2 = _flags(inf1, n, "inf1"), _flags(inf2, n, "inf2")
        ok = np.empty(n // k, dtype=np.uint8)
        allok = ctypes.c_int(1)
        self._chk(self._lib.zkp_pairing_check_batch(self._h, _ptr(g1), _ptr(g2), _ptr(i1), _ptr(i2), n // k, k, _ptr(ok), ctypes.byref(allok)))
        return ok, bool(allok.value)

    # ---- the whole batch as ONE product check (one shared final exponentiation)
    def miller_product(self, g1, g2, inf1=None, inf2=None):
        """multi_miller_loop over ALL pairs of the batch -> (72,) MillerLoopResult"""
        if _is_torch(g1):
            import torch
            self._t_pairs(g1, g2, inf1, inf2)
            out = torch.empty(72, dtype=g1.dtype, device=g1.device)
            self._chk(self._lib.zkp_miller_product_dev(self._h, self._tp(g1), self._tp(g2), self._tp(inf1), self._tp(inf2), g1.numel() // 12,
                                                       self._tp(out), self._stream()))
            return out
        g1, g2 = _np(g1, 12), _np(g2, 24)
        n = g1.shape[0]
        if g2.shape[0] != n:
            raise ValueError("g1 and g2 hold different numbers of points")
        i1, i2 = _flags(inf1, n, "inf1"), _flags(inf2, n, "inf2")
        out = np.empty(72, dtype=np.uint64)
        self._chk(self._lib.zkp_miller_product(self._h, _ptr(g1), _ptr(g2), _ptr(i1), _ptr(i2), n, _ptr(out)))
        return out

    def fp12_product(self, f):
        """f_0 * f_1 * ... * f_n-1 of (n,72) Fp12 values -> (72,)"""
        if _is_torch(f):
            import torch
            self._t_check(f, 72, "f")
            out = torch.empty(72, dtype=f.dtype, device=f.device)
            self._chk(self._lib.zkp_fp12_product_dev(self._h, self._tp(f), f.numel() // 72, self._tp(out), self._stream()))
            return out
        f = _np(f, 72)
        out = np.empty(72, dtype=np.uint64)
        self._chk(self._lib.zkp_fp12_product(self._h, _ptr(f), f.shape[0], _ptr(out)))
        return out

    def pairing_product_check(self, g1, g2, inf1=None, inf2=None):
        """-> (Gt (72,), is_one): prod_i e(g1[i], g2[i]) == Gt::identity() with one final exponentiation.
        Device tensors return (Gt tensor, int32 tensor(1,)) without synchronising."""
        if _is_torch(g1):
            import torch
            self._t_pairs(g1, g2, inf1, inf2)
            gt = torch.empty(72, dtype=g1.dtype, device=g1.device)
            one = torch.empty(1, dtype=torch.int32, device=g1.device)
            self._chk(self._lib.zkp_pairing_product_check_dev(self._h, self._tp(g1), self._tp(g2), self._tp(inf1), self._tp(inf2), g1.numel() // 12,
                                                              self._tp(gt), self._tp(one), self._stream()))
            return gt, one
        g1, g2 = _np(g1, 12), _np(g2, 24)
        n = g1.shape[0]
        if g2.shape[0] != n:
            raise ValueError("g1 and g2 hold different numbers of points")
        i1, i2 = _flags(inf1, n, "inf1"), _flags(inf2, n, "inf2")
        gt = np.empty(72, dtype=np.uint64)
        one = ctypes.c_int(0)
        self._chk(self._lib.zkp_pairing_product_check(self._h, _ptr(g1), _ptr(g2), _ptr(i1), _ptr(i2), n, _ptr(gt), ctypes.byref(one)))
        return gt, bool(one.value)

    def g1_is_valid(self, g1, inf=None):
        if _is_torch(g1):
            return self._valid_t(g1, inf, 1)
        g1 = _np(g1, 12)
        i = _flags(inf, g1.shape[0], "inf")
        st = np.empty(g1.shape[0], dtype=np.uint8)
        self._chk(self._lib.zkp_g1_is_valid_batch(self._h, _ptr(g1), _ptr(i), g1.shape[0], _ptr(st)))
        return st

    def g2_is_valid(self, g2, inf=None):
        if _is_torch(g2):
            return self._valid_t(g2, inf, 2)
        g2 = _np(g2, 24)
        i = _flags(inf, g2.shape[0], "inf")
        st = np.empty(g2.shape[0], dtype=np.uint8)
        self._chk(self._lib.zkp_g2_is_valid_batch(self._h, _ptr(g2), _ptr(i), g2.shape[0], _ptr(st)))
        return st

    def g1_mul(self, base, scalars):
        """[k_i] base_i; base (12,) broadcasts. -> (points (n,12), inf (n,))"""
        if _is_torch(scalars):
            return self._mul_t(base, scalars, 1)
        sc = _np(scalars, 4)
        base = _np(base, 12)
        n = sc.shape[0]
        stride = 0 if base.shape[0] == 1 and n != 1 else 12
        if stride and base.shape[0] != n:
            raise ValueError("base points and scalars differ in number")
        out, oi = np.empty((n, 12), dtype=np.uint64), np.empty(n, dtype=np.uint8)
        self._chk(self._lib.zkp_g1_mul_batch(self._h, _ptr(base), stride, _ptr(sc), n, _ptr(out), _ptr(oi)))
        return out, oi

    def g2_mul(self, base, scalars):
        if _is_torch(scalars):
            return self._mul_t(base, scalars, 2)
        sc = _np(scalars, 4)
        base = _np(base, 24)
        n = sc.shape[0]
        stride = 0 if base.shape[0] == 1 and n != 1 else 24
        if stride and base.shape[0] != n:
            raise ValueError("base points and scalars differ in number")
        out, oi = np.empty((n, 24), dtype=np.uint64), np.empty(n, dtype=np.uint8)
        self._chk(self._lib.zkp_g2_mul_batch(self._h, _ptr(base), stride, _ptr(sc), n, _ptr(out), _ptr(oi)))
        return out, oi

    def g1_add(self, a, b, inf_a=None, inf_b=None):
        """a[i] + b[i] (G1Affine Add); -> (points (n,12), inf (n,)).  torch tensors stay on the GPU (the engine's stream)."""
        return self._add(a, b, inf_a, inf_b, 1)

    def g2_add(self, a, b, inf_a=None, inf_b=None):
        return self._add(a, b, inf_a, inf_b, 2)

    def g1_msm(self, points, scalars, n_msm=1, inf=None, shared_bases=False):
        """n_msm sums of m = len(scalars) / n_msm terms: out[j] = sum_i [k_(j,i)] P_(j,i); points hold m (shared_bases) or
        m * n_msm entries.  -> (points (n_msm,12), inf (n_msm,))"""
        return self._msm(points, scalars, n_msm, inf, shared_bases, 1)

    def g2_msm(self, points, scalars, n_msm=1, inf=None, shared_bases=False):
        return self._msm(points, scalars, n_msm, inf, shared_bases, 2)

    def _add(self, a, b, inf_a, inf_b, which):
        cols = 12 if which == 1 else 24
        if _is_torch(a):
            import torch
            self._t_check(a, cols, "a")
            self._t_check(b, cols, "b")
            n = a.numel() // cols
            if b.numel() != a.numel():
                raise ValueError("a and b differ in number of points")
            self._t_bytes(inf_a, n, "inf_a"), self._t_bytes(inf_b, n, "inf_b")
            out = torch.empty((n, cols), dtype=a.dtype, device=a.device)
            oi = torch.empty(n, dtype=torch.uint8, device=a.device)
            fn = self._lib.zkp_g1_add_batch_dev if which == 1 else self._lib.zkp_g2_add_batch_dev
            self._chk(fn(self._h, self._tp(a), self._tp(inf_a), self._tp(b), self._tp(inf_b), n, self._tp(out), self._tp(oi), self._stream()))
            return out, oi
        a, b = _np(a, cols), _np(b, cols)
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("a and b differ in number of points")
        ia, ib = _flags(inf_a, n, "inf_a"), _flags(inf_b, n, "inf_b")
        out, oi = np.empty((n, cols), dtype=np.uint64), np.empty(n, dtype=np.uint8)
        fn = self._lib.zkp_g1_add_batch if which == 1 else self._lib.zkp_g2_add_batch
        self._chk(fn(self._h, _ptr(a), _ptr(ia), _ptr(b), _ptr(ib), n, _ptr(out), _ptr(oi)))
        return out, oi

    def _msm_shape(self, n_pts, n_sc, n_msm, shared):
        if n_msm < 1 or n_sc % n_msm:
            raise ValueError("%d scalars do not split into %d sums" % (n_sc, n_msm))
        m = n_sc // n_msm
        if n_pts != (m if shared else n_sc):
            raise ValueError("%d points for %d sums of %d terms (shared_bases=%s)" % (n_pts, n_msm, m, bool(shared)))
        return m

    def _msm(self, points, scalars, n_msm, inf, shared, which):
        cols = 12 if which == 1 else 24
        n_msm = int(n_msm)
        if _is_torch(scalars):
            import torch
            self._t_check(scalars, 4, "scalars")
            self._t_check(points, cols, "points")
            m = self._msm_shape(points.numel() // cols, scalars.numel() // 4, n_msm, shared)
            self._t_bytes(inf, points.numel() // cols, "inf")
            out = torch.empty((n_msm, cols), dtype=scalars.dtype, device=scalars.device)
            oi = torch.empty(n_msm, dtype=torch.uint8, device=scalars.device)
            fn = self._lib.zkp_g1_msm_batch_dev if which == 1 else self._lib.zkp_g2_msm_batch_dev
            self._chk(fn(self._h, self._tp(points), self._tp(inf), self._tp(scalars), m, n_msm, 1 if shared else 0, self._tp(out), self._tp(oi),
                         self._stream()))
            return out, oi
        pts, sc = _np(points, cols), _np(scalars, 4)
        m = self._msm_shape(pts.shape[0], sc.shape[0], n_msm, shared)
        i = _flags(inf, pts.shape[0], "inf")
        out, oi = np.empty((n_msm, cols), dtype=np.uint64), np.empty(n_msm, dtype=np.uint8)
        fn = self._lib.zkp_g1_msm_batch if which == 1 else self._lib.zkp_g2_msm_batch
        self._chk(fn(self._h, _ptr(pts), _ptr(i), _ptr(sc), m, n_msm, 1 if shared else 0, _ptr(out), _ptr(oi)))
        return out, oi

    # ---- batch verification by random linear combination
    def g1_mul_endo(self, base, ab, inf=None):
        """[a_i] P_i + [b_i] (beta x_i, -y_i), ab (n, 2) uint64 = (a_i, b_i): for P_i in G1 this is [a_i + b_i z^2] P_i (z the BLS parameter).
        -> (points (n,12), inf (n,)).  torch tensors stay on the GPU (the engine's stream)."""
        if _is_torch(base):
            import torch
            self._t_check(base, 12, "base")
            n = base.numel() // 12
            self._t_check(ab, 2, "ab")
            if ab.numel() != 2 * n:
                raise ValueError("ab holds %d pairs for %d points" % (ab.numel() // 2, n))
            self._t_bytes(inf, n, "inf")
            out = torch.empty((n, 12), dtype=base.dtype, device=base.device)
            oi = torch.empty(n, dtype=torch.uint8, device=base.device)
            self._chk(self._lib.zkp_g1_mul_endo_batch_dev(self._h, self._tp(base), self._tp(inf), self._tp(ab), n, self._tp(out), self._tp(oi),
                                                          self._stream()))
            return out, oi
        base, ab = _np(base, 12), _np(ab, 2)
        n = base.shape[0]
        if ab.shape[0] != n:
            raise ValueError("ab holds %d pairs for %d points" % (ab.shape[0], n))
        i = _flags(inf, n, "inf")
        out, oi = np.empty((n, 12), dtype=np.uint64), np.empty(n, dtype=np.uint8)
        self._chk(self._lib.zkp_g1_mul_endo_batch(self._h, _ptr(base), _ptr(i), _ptr(ab), n, _ptr(out), _ptr(oi)))
        return out, oi

    @staticmethod
    def rlc_random(n):
        """(n, 2) uint64 scalars (a_c, b_c) for pairing_check_rlc from the operating system's CSPRNG (os.urandom), no pair (0, 0)"""
        import os
        r = np.frombuffer(os.urandom(16 * n), dtype=np.uint64).reshape(n, 2).copy()
        while n and (r == 0).all(axis=1).any():
            z = (r == 0).all(axis=1)
            r[z] = np.frombuffer(os.urandom(16 * int(z.sum())), dtype=np.uint64).reshape(-1, 2)
        return r

    def pairing_check_rlc(self, g1, g2, k, *, col_g1=None, fixed_g2=None, col_g2=None, fixed_g1=None, inf1=None, inf2=None, col_inf1=None,
                          fixed_inf2=None, col_inf2=None, fixed_inf1=None, rand=None, points_checked=False, locate=False):
        """n independent pairing checks verified as ONE (zkp_pairing_check_batch_rlc): check c is the product of its k free pairs
        (g1[c k + j], g2[c k + j]), its s2 pairs (col_g1[c s2 + j], fixed_g2[j]) and its s1 pairs (fixed_g1[j], col_g2[c s1 + j]).
        True iff prod_c (check c)^(a_c + b_c z^2) == 1, every point is valid (unless points_checked) and no (a_c, b_c) is zero;
        a batch with a failing check passes with probability <= 2^-128.  rand (n, 2) uint64: the scalars, by default fresh from
        os.urandom (rlc_random) - never a seeded generator.  Host arrays return a bool; resident torch tensors an int32 tensor (1,)
        without synchronising.  locate=True returns (all_ok, ok bytes (n,)): when the batch fails, the per-check flags of
        pairing_check on the expanded checks (ANDed with the points' validity unless points_checked)."""
        torch_in = any(_is_torch(x) for x in (g1, col_g1, col_g2))
        cols = lambda x, w: 0 if x is None else (x.numel() if _is_torch(x) else np.asarray(x).size) // w
        k = int(k)
        s2, s1 = cols(fixed_g2, 24), cols(fixed_g1, 12)
        if k < 0 or (k and g1 is None):
            raise ValueError("k = %d free pairs per check without g1 / g2" % k)
        if k:
            n, n_from = cols(g1, 12) // k, cols(g1, 12)
            if n_from % k:
                raise ValueError("%d G1 points is not a multiple of k = %d" % (n_from, k))
        elif s2:
            n = cols(col_g1, 12) // s2
        elif s1:
            n = cols(col_g2, 24) // s1
        else:
            n = 0
        want = {"g1": (g1, 12, n * k), "g2": (g2, 24, n * k), "col_g1": (col_g1, 12, n * s2), "col_g2": (col_g2, 24, n * s1)}
        for name, (x, w, rows) in want.items():
            if rows and cols(x, w) != rows:
                raise ValueError("%s holds %d points, %d expected" % (name, cols(x, w), rows))
        if (s2 and col_g1 is None) or (s1 and col_g2 is None):
            raise ValueError("a fixed column without its per-check points")
        if n == 0:
            return (True, np.zeros(0, dtype=np.uint8)) if locate else True
        if rand is None:
            rand = self.rlc_random(n)
        flags = _lib.RLC_POINTS_CHECKED if points_checked else 0
        arrays = [("g1", g1, 12, n * k), ("g2", g2, 24, n * k), ("inf1", inf1, None, n * k), ("inf2", inf2, None, n * k),
                  ("col_g1", col_g1, 12, n * s2), ("col_inf1", col_inf1, None, n * s2), ("fixed_g2", fixed_g2, 24, s2), ("fixed_inf2", fixed_inf2, None, s2),
                  ("col_g2", col_g2, 24, n * s1), ("col_inf2", col_inf2, None, n * s1), ("fixed_g1", fixed_g1, 12, s1), ("fixed_inf1", fixed_inf1, None, s1)]
        b = _lib.RlcBatch(n_checks=n, k=k, s2=s2, s1=s1)
        keep = []
        if torch_in:
            import torch
            dev = torch.device("cuda", self.device)
            for name, x, w, rows in arrays:
                if x is None or not rows:
                    continue
                if w is None:
                    self._t_bytes(x, rows, name)
                else:
                    self._t_check(x, w, name, rows=rows)
                setattr(b, name, x.data_ptr())
            if not _is_torch(rand):
                rand = torch.from_numpy(np.ascontiguousarray(rand, dtype=np.uint64).reshape(-1).view(np.int64)).to(dev)
            self._t_check(rand, 2, "rand", rows=n)
            all_ok = torch.empty(1, dtype=torch.int32, device=dev)
            self._chk(self._lib.zkp_pairing_check_batch_rlc_dev(self._h, ctypes.byref(b), self._tp(rand), flags, self._tp(all_ok), self._stream()))
            if not locate:
                return all_ok
            ok = bool(all_ok.item())
            host = lambda x: None if x is None else (x.cpu().numpy() if _is_torch(x) else x)
            g1, g2, inf1, inf2, col_g1, col_inf1, fixed_g2, fixed_inf2, col_g2, col_inf2, fixed_g1, fixed_inf1 = [host(a[1]) for a in arrays]
        else:
            for name, x, w, rows in arrays:
                if x is None or not rows:
                    continue
                a = _flags(x, rows, name) if w is None else _np(x, w)
                if w is not None and a.shape[0] != rows:
                    raise ValueError("%s holds %d points, %d expected" % (name, a.shape[0], rows))
                keep.append(a)
                setattr(b, name, a.ctypes.data)
            r = _np(rand, 2)
            if r.shape[0] != n:
                raise ValueError("rand holds %d pairs for %d checks" % (r.shape[0], n))
            res = ctypes.c_int(0)
            self._chk(self._lib.zkp_pairing_check_batch_rlc(self._h, ctypes.byref(b), _ptr(r), flags, ctypes.byref(res)))
            ok = bool(res.value)
            if not locate:
                return ok
        if ok:
            return True, np.ones(n, dtype=np.uint8)
        e1, e2, f1, f2, kk = self._rlc_expand(n, k, s1, s2, g1, g2, inf1, inf2, col_g1, col_inf1, fixed_g2, fixed_inf2, col_g2, col_inf2, fixed_g1,
                                              fixed_inf1)
        per, _ = self.pairing_check(e1, e2, kk, f1, f2)
        if not points_checked:
            bad = (self.g1_is_valid(e1, f1) | self.g2_is_valid(e2, f2)).reshape(n, kk).any(axis=1)
            per[bad] = 0
        return False, per

    @staticmethod
    def _rlc_expand(n, k, s1, s2, g1, g2, inf1, inf2, col_g1, col_inf1, fixed_g2, fixed_inf2, col_g2, col_inf2, fixed_g1, fixed_inf1):
        """the checks of a pairing_check_rlc batch as k + s2 + s1 consecutive pairs each (host arrays)"""
        kk = k + s2 + s1
        e1, e2 = np.zeros((n, kk, 12), dtype=np.uint64), np.zeros((n, kk, 24), dtype=np.uint64)
        f1, f2 = np.zeros((n, kk), dtype=np.uint8), np.zeros((n, kk), dtype=np.uint8)
        fl = lambda x, shape: 0 if x is None else np.asarray(x, dtype=np.uint8).reshape(shape)
        if k:
            e1[:, :k], e2[:, :k] = _np(g1, 12).reshape(n, k, 12), _np(g2, 24).reshape(n, k, 24)
            f1[:, :k], f2[:, :k] = fl(inf1, (n, k)), fl(inf2, (n, k))
        if s2:
            e1[:, k:k + s2], e2[:, k:k + s2] = _np(col_g1, 12).reshape(n, s2, 12), _np(fixed_g2, 24)[None]
            f1[:, k:k + s2], f2[:, k:k + s2] = fl(col_inf1, (n, s2)), fl(fixed_inf2, (1, s2))
        if s1:
            e1[:, k + s2:], e2[:, k + s2:] = _np(fixed_g1, 12)[None], _np(col_g2, 24).reshape(n, s1, 24)
            f1[:, k + s2:], f2[:, k + s2:] = fl(fixed_inf1, (1, s1)), fl(col_inf2, (n, s1))
        return e1.reshape(-1, 12), e2.reshape(-1, 24), f1.reshape(-1), f2.reshape(-1), kk

    # ---- the scalar field Fr (4 u64 per element, canonical), the Fr fold and the batched Groth16 verifier
    FR_OPS = {"mul": 0, "add": 1, "sub": 2, "neg": 3, "square": 4, "invert": 5}

    def fr_op(self, op, a, b=None):
        """out[i] = a[i] op b[i] in Fr (zkp_fr_op_batch): op a name in FR_OPS or its number; neg / square / invert ignore b; 0 inverts to
        0.  numpy (n, 4) uint64 in, the same out; resident torch tensors stay on the GPU (the current stream)."""
        op = int(self.FR_OPS.get(op, op))
        if _is_torch(a):
            import torch
            self._t_check(a, 4, "a")
            n = a.numel() // 4
            if b is not None:
                self._t_check(b, 4, "b", rows=n)
            out = torch.empty((n, 4), dtype=a.dtype, device=a.device)
            self._chk(self._lib.zkp_fr_op_batch_dev(self._h, op, self._tp(a), self._tp(b), n, self._tp(out), self._stream()))
            return out
        a = _np(a, 4)
        b = None if b is None else _np(b, 4)
        if b is not None and b.shape != a.shape:
            raise ValueError("fr_op: operand shapes differ")
        out = np.empty_like(a)
        self._chk(self._lib.zkp_fr_op_batch(self._h, op, _ptr(a), _ptr(b), a.shape[0], _ptr(out)))
        return out

    def fr_from_wide(self, data):
        """64 little-endian bytes per element -> the 512-bit integer mod r (Fr::from_bytes_wide), (n, 4) uint64; a uint8 array / bytes, or
        a resident uint8 tensor"""
        if _is_torch(data):
            import torch
            self._t_check(data, 64, "bytes", dtypes=(torch.uint8,))
            n = data.numel() // 64
            out = torch.empty((n, 4), dtype=torch.int64, device=data.device)
            self._chk(self._lib.zkp_fr_from_wide_batch_dev(self._h, self._tp(data), n, self._tp(out), self._stream()))
            return out
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        if buf.size % 64:
            raise ValueError("byte string is not a multiple of 64 bytes")
        out = np.empty((buf.size // 64, 4), dtype=np.uint64)
        self._chk(self._lib.zkp_fr_from_wide_batch(self._h, _ptr(buf), buf.size // 64, _ptr(out)))
        return out

    def fr_fold(self, w, x, l=None):
        """(out (l, 4), sum_w (4,)): out[i] = sum_c w[c] x[c][i] mod r and sum_w = sum_c w[c] mod r (zkp_fr_fold_batch); w (n, 4), x (n, l, 4)
        or (n l, 4) with l given.  Resident torch tensors stay on the GPU."""
        if _is_torch(w):
            import torch
            self._t_check(w, 4, "w")
            n = w.numel() // 4
            self._t_check(x, 4, "x")
            l = (x.shape[1] if x.dim() == 3 else (x.numel() // 4 // n if n else 0)) if l is None else int(l)
            if x.numel() != n * l * 4:
                raise ValueError("x holds %d elements for %d rows of %d" % (x.numel() // 4, n, l))
            out = torch.empty((l, 4), dtype=w.dtype, device=w.device)
            sw = torch.empty(4, dtype=w.dtype, device=w.device)
            self._chk(self._lib.zkp_fr_fold_batch_dev(self._h, self._tp(w), self._tp(x) if n * l else None, n, l, self._tp(out) if l else None,
                                                      self._tp(sw), self._stream()))
            return out, sw
        w = _np(w, 4)
        n = w.shape[0]
        x = np.ascontiguousarray(x, dtype=np.uint64)
        l = (x.shape[1] if x.ndim == 3 else (x.size // 4 // n if n else 0)) if l is None else int(l)
        if x.size != n * l * 4:
            raise ValueError("x holds %d elements for %d rows of %d" % (x.size // 4, n, l))
        out, sw = np.empty((l, 4), dtype=np.uint64), np.empty(4, dtype=np.uint64)
        self._chk(self._lib.zkp_fr_fold_batch(self._h, _ptr(w), _ptr(x) if n * l else None, n, l, _ptr(out) if l else None, _ptr(sw)))
        return out, sw

    def groth16_verify_batch(self, alpha_g1, beta_g2, gamma_g2, delta_g2, ic, a, b, c, inputs, *, inf_a=None, inf_b=None, inf_c=None, rand=None,
                             points_checked=False, vk_checked=False):
        """n Groth16 proofs against one verifying key as ONE check (zkp_groth16_verify_batch): key points alpha (12,), beta / gamma /
        delta (24,), ic (n_inputs + 1, 12); proofs a (n, 12), b (n, 24), c (n, 12); inputs (n, n_inputs, 4) canonical Fr elements.  True
        iff the random combination holds, every point is valid (unless points_checked / vk_checked), every input is below r and no
        (a_c, b_c) is zero; a batch with an invalid proof passes with probability <= 2^-128.  rand (n, 2) uint64, by default fresh from
        os.urandom (rlc_random) - never a seeded generator.  Host arrays return a bool; resident torch tensors (all of them) an int32
        tensor (1,) without synchronising."""
        cnt = lambda x, w: (x.numel() if _is_torch(x) else np.asarray(x).size) // w
        n, l = cnt(a, 12), cnt(ic, 12) - 1
        if l < 0:
            raise ValueError("ic holds no point")
        if n == 0:
            return True
        if rand is None:
            rand = self.rlc_random(n)
        flags = (_lib.GROTH16_POINTS_CHECKED if points_checked else 0) | (_lib.GROTH16_VK_CHECKED if vk_checked else 0)
        vk_arrays = [("alpha_g1", alpha_g1, 12, 1), ("beta_g2", beta_g2, 24, 1), ("gamma_g2", gamma_g2, 24, 1), ("delta_g2", delta_g2, 24, 1),
                     ("ic", ic, 12, l + 1)]
        b_arrays = [("a", a, 12, n), ("inf_a", inf_a, None, n), ("b", b, 24, n), ("inf_b", inf_b, None, n), ("c", c, 12, n), ("inf_c", inf_c, None, n),
                    ("inputs", inputs, 4, n * l)]
        vk = _lib.Groth16Vk(n_inputs=l)
        bt = _lib.Groth16Batch(n=n)
        keep = []
        if _is_torch(a):
            import torch
            dev = torch.device("cuda", self.device)
            for rec, arrays in ((vk, vk_arrays), (bt, b_arrays)):
                for name, x, w, rows in arrays:
                    if x is None or not rows:
                        continue
                    if w is None:
                        self._t_bytes(x, rows, name)
                    else:
                        self._t_check(x, w, name, rows=rows)
                        if x.numel() != rows * w:
                            raise ValueError("%s holds %d elements, %d expected" % (name, x.numel() // w, rows))
                    setattr(rec, name, x.data_ptr())
            if not _is_torch(rand):
                rand = torch.from_numpy(np.ascontiguousarray(rand, dtype=np.uint64).reshape(-1).view(np.int64)).to(dev)
            self._t_check(rand, 2, "rand", rows=n)
            all_ok = torch.empty(1, dtype=torch.int32, device=dev)
            self._chk(self._lib.zkp_groth16_verify_batch_dev(self._h, ctypes.byref(vk), ctypes.byref(bt), self._tp(rand), flags, self._tp(all_ok),
                                                             self._stream()))
            return all_ok
        for rec, arrays in ((vk, vk_arrays), (bt, b_arrays)):
            for name, x, w, rows in arrays:
                if x is None or not rows:
                    continue
                arr = _flags(x, rows, name) if w is None else _np(x, w)
                if w is not None and arr.shape[0] != rows:
                    raise ValueError("%s holds %d elements, %d expected" % (name, arr.shape[0], rows))
                keep.append(arr)
                setattr(rec, name, arr.ctypes.data)
        r = _np(rand, 2)
        if r.shape[0] != n:
            raise ValueError("rand holds %d pairs for %d proofs" % (r.shape[0], n))
        res = ctypes.c_int(0)
        self._chk(self._lib.zkp_groth16_verify_batch(self._h, ctypes.byref(vk), ctypes.byref(bt), _ptr(r), flags, ctypes.byref(res)))
        return bool(res.value)

    def fr_invert(self, a, out=None):
        """out[i] = a[i]^-1 in Fr, 0 for 0 (zkp_fr_invert_batch: Montgomery's trick, one power per call; the same bits as
        fr_op("invert")).  numpy (n, 4) uint64 in, the same out; resident torch tensors stay on the GPU (the current stream), and
        out=a inverts in place."""
        if _is_torch(a):
            import torch
            self._t_check(a, 4, "a")
            n = a.numel() // 4
            if out is None:
                out = torch.empty((n, 4), dtype=a.dtype, device=a.device)
            else:
                self._t_check(out, 4, "out", rows=n)
            self._chk(self._lib.zkp_fr_invert_batch_dev(self._h, self._tp(a), n, self._tp(out), self._stream()))
            return out
        a = _np(a, 4)
        res = np.empty_like(a)
        self._chk(self._lib.zkp_fr_invert_batch(self._h, _ptr(a), a.shape[0], _ptr(res)))
        return res

    def fr_eval(self, evals, z, log2_n, bitrev=False):
        """(n_poly, 4): polynomial j, given by its N = 2^log2_n evaluations evals[j] over the N-th roots of unity w^i (in bit-reversed
        order with bitrev, as blobs are stored), at the point z[j] (zkp_fr_eval_batch: the barycentric formula; z[j] = w^i gives
        evals[j][i]).  evals (n_poly, N, 4) or (n_poly N, 4), z (n_poly, 4), canonical.  Resident torch tensors stay on the GPU."""
        log2_n, flags = int(log2_n), _lib.FR_EVAL_BITREV if bitrev else 0
        if _is_torch(evals):
            import torch
            self._t_check(z, 4, "z")
            n_poly = z.numel() // 4
            self._t_check(evals, 4, "evals")
            if log2_n < 0 or evals.numel() != (n_poly << log2_n) * 4:
                raise ValueError("evals hold %d elements for %d polynomials of 2^%d" % (evals.numel() // 4, n_poly, log2_n))
            out = torch.empty((n_poly, 4), dtype=z.dtype, device=z.device)
            self._chk(self._lib.zkp_fr_eval_batch_dev(self._h, self._tp(evals), self._tp(z), n_poly, log2_n, flags, self._tp(out), self._stream()))
            return out
        z = _np(z, 4)
        n_poly = z.shape[0]
        evals = np.ascontiguousarray(evals, dtype=np.uint64)
        if log2_n < 0 or evals.size != (n_poly << log2_n) * 4:
            raise ValueError("evals hold %d elements for %d polynomials of 2^%d" % (evals.size // 4, n_poly, log2_n))
        out = np.empty((n_poly, 4), dtype=np.uint64)
        self._chk(self._lib.zkp_fr_eval_batch(self._h, _ptr(evals), _ptr(z), n_poly, log2_n, flags, _ptr(out)))
        return out

    def fr_ntt(self, x, log2_n, inverse=False, bitrev=False, coset=False, out=None):
        """The NTT of n_poly polynomials of N = 2^log2_n coefficients each over the N-th roots of unity w^i (zkp_fr_ntt_batch):
        out[j][i] = sum_k x[j][k] (s w^i)^k, s = 7 with coset; with bitrev the evaluation side is bit-reversed (slot i belongs to
        w^bitrev(i), the order fr_eval's bitrev reads); inverse is the exact inverse map under the same other flags.  x (n_poly, N, 4)
        or (n_poly N, 4) uint64, canonical; the result has x's shape.  Resident torch tensors stay on the GPU (the current stream),
        and out=x transforms in place."""
        log2_n = int(log2_n)
        flags = (_lib.NTT_INVERSE if inverse else 0) | (_lib.NTT_BITREV if bitrev else 0) | (_lib.NTT_COSET if coset else 0)
        if _is_torch(x):
            import torch
            self._t_check(x, 4, "x")
            n_el = x.numel() // 4
            if log2_n < 0 or log2_n > 63 or n_el % (1 << log2_n):
                raise ValueError("x holds %d elements: no whole number of polynomials of 2^%d" % (n_el, log2_n))
            if out is None:
                out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            else:
                self._t_check(out, 4, "out", rows=n_el)
            self._chk(self._lib.zkp_fr_ntt_batch_dev(self._h, self._tp(x), n_el >> log2_n, log2_n, flags, self._tp(out), self._stream()))
            return out
        x = np.ascontiguousarray(x, dtype=np.uint64)
        n_el = x.size // 4
        if log2_n < 0 or log2_n > 63 or x.size % 4 or n_el % (1 << log2_n):
            raise ValueError("x holds %d elements: no whole number of polynomials of 2^%d" % (n_el, log2_n))
        if out is None:
            out = np.empty_like(x)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.uint64 and out.flags.c_contiguous and out.size == x.size):
            raise ValueError("out must be a C-contiguous uint64 array of x's size")
        self._chk(self._lib.zkp_fr_ntt_batch(self._h, _ptr(x), n_el >> log2_n, log2_n, flags, _ptr(out)))
        return out

    def kzg_open(self, lagrange_g1, evals, z, log2_n, bitrev=False):
        """KZG openings on the GPU (zkp_kzg_open_batch): polynomial j, given by its N = 2^log2_n evaluations evals[j] (bit-reversed
        order with bitrev), at the point z[j], against the Lagrange setup lagrange_g1 (N, 12) in the SAME order as the evaluations.
        -> (y (n, 4), proofs (n, 12), inf (n,)): y[j] = f_j(z[j]) and the proof [(f_j(tau) - y[j]) / (tau - z[j])] g1 that
        kzg_verify_batch consumes.  The setup points are trusted (check them once with g1_is_valid).  Resident torch tensors (all
        three) stay on the GPU."""
        log2_n, flags = int(log2_n), _lib.FR_EVAL_BITREV if bitrev else 0
        if log2_n < 0 or log2_n > 63:
            raise ValueError("log2_n out of range")
        if _is_torch(evals):
            import torch
            self._t_check(z, 4, "z")
            n = z.numel() // 4
            self._t_check(evals, 4, "evals", rows=n << log2_n)
            self._t_check(lagrange_g1, 12, "lagrange_g1", rows=1 << log2_n)
            y = torch.empty((n, 4), dtype=z.dtype, device=z.device)
            proof = torch.empty((n, 12), dtype=z.dtype, device=z.device)
            inf = torch.empty(n, dtype=torch.uint8, device=z.device)
            self._chk(self._lib.zkp_kzg_open_batch_dev(self._h, self._tp(lagrange_g1), self._tp(evals), self._tp(z), n, log2_n, flags, self._tp(y),
                                                       self._tp(proof), self._tp(inf), self._stream()))
            return y, proof, inf
        z = _np(z, 4)
        n = z.shape[0]
        evals = np.ascontiguousarray(evals, dtype=np.uint64)
        setup = _np(lagrange_g1, 12)
        if evals.size != (n << log2_n) * 4:
            raise ValueError("evals hold %d elements for %d polynomials of 2^%d" % (evals.size // 4, n, log2_n))
        if setup.shape[0] != 1 << log2_n:
            raise ValueError("the setup holds %d points for polynomials of 2^%d" % (setup.shape[0], log2_n))
        y, proof, inf = np.empty((n, 4), dtype=np.uint64), np.empty((n, 12), dtype=np.uint64), np.empty(n, dtype=np.uint8)
        self._chk(self._lib.zkp_kzg_open_batch(self._h, _ptr(setup), _ptr(evals), _ptr(z), n, log2_n, flags, _ptr(y), _ptr(proof), _ptr(inf)))
        return y, proof, inf

    # ------------------------------------------------------------------ the G1 NTT and FK20 (include/zkp_fk20.h)
    def g1_ntt(self, points, log2_n, inverse=False, bitrev=False, inf=None, out=None, out_inf=None):
        """The NTT of n_vec vectors of N = 2^log2_n G1 points each (zkp_g1_ntt_batch): out[j][i] = sum_k [w^(i k)] points[j][k] with the
        root of fr_ntt; inverse and bitrev mean what they mean there.  points (n_vec N, 12), inf optional flags (n_vec N,).
        -> (out (n_vec N, 12), out_inf (n_vec N,)); the identity is (0, 1) with its flag set.  The points are trusted (on the curve, in
        the subgroup).  Resident torch tensors stay on the GPU (the current stream); out=points, out_inf=inf transforms in place."""
        log2_n = int(log2_n)
        flags = (_lib.NTT_INVERSE if inverse else 0) | (_lib.NTT_BITREV if bitrev else 0)
        if log2_n < 0 or log2_n > 63:
            raise ValueError("log2_n out of range")
        if _is_torch(points):
            import torch
            self._t_check(points, 12, "points")
            n = points.numel() // 12
            if n % (1 << log2_n):
                raise ValueError("%d points: no whole number of vectors of 2^%d" % (n, log2_n))
            self._t_bytes(inf, n, "inf")
            if out is None:
                out = torch.empty((n, 12), dtype=points.dtype, device=points.device)
            if out_inf is None:
                out_inf = torch.empty(n, dtype=torch.uint8, device=points.device)
            self._t_check(out, 12, "out", rows=n), self._t_bytes(out_inf, n, "out_inf")
            self._chk(self._lib.zkp_g1_ntt_batch_dev(self._h, self._tp(points), self._tp(inf), n >> log2_n, log2_n, flags, self._tp(out), self._tp(out_inf),
                                                     self._stream()))
            return out, out_inf
        pts = _np(points, 12)
        n = pts.shape[0]
        if n % (1 << log2_n):
            raise ValueError("%d points: no whole number of vectors of 2^%d" % (n, log2_n))
        inf = _flags(inf, n, "g1_ntt")
        if out is None:
            out = np.empty((n, 12), dtype=np.uint64)
        if out_inf is None:
            out_inf = np.empty(n, dtype=np.uint8)
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint64 and out.flags.c_contiguous and out.size == n * 12 and
                isinstance(out_inf, np.ndarray) and out_inf.dtype == np.uint8 and out_inf.flags.c_contiguous and out_inf.size == n):
            raise ValueError("out / out_inf must be C-contiguous uint64 / uint8 arrays of the input's size")
        self._chk(self._lib.zkp_g1_ntt_batch(self._h, _ptr(pts), _ptr(inf), n >> log2_n, log2_n, flags, _ptr(out), _ptr(out_inf)))
        return out, out_inf

    def kzg_fk20_setup(self, monomial_g1, log2_n):
        """(setup (2N, 12), inf (2N,)) for kzg_fk20, from the monomial setup monomial_g1[k] = [tau^k] g1, k < N = 2^log2_n
        (zkp_kzg_fk20_setup): computed once per setup.  The points are trusted.  A resident torch tensor stays on the GPU."""
        log2_n = int(log2_n)
        if log2_n < 0 or log2_n > 63:
            raise ValueError("log2_n out of range")
        big_n = 1 << log2_n
        if _is_torch(monomial_g1):
            import torch
            self._t_check(monomial_g1, 12, "monomial_g1", rows=big_n)
            out = torch.empty((2 * big_n, 12), dtype=monomial_g1.dtype, device=monomial_g1.device)
            out_inf = torch.empty(2 * big_n, dtype=torch.uint8, device=monomial_g1.device)
            self._chk(self._lib.zkp_kzg_fk20_setup_dev(self._h, self._tp(monomial_g1), log2_n, self._tp(out), self._tp(out_inf), self._stream()))
            return out, out_inf
        mono = _np(monomial_g1, 12)
        if mono.shape[0] != big_n:
            raise ValueError("the monomial setup holds %d points for polynomials of 2^%d" % (mono.shape[0], log2_n))
        out, out_inf = np.empty((2 * big_n, 12), dtype=np.uint64), np.empty(2 * big_n, dtype=np.uint8)
        self._chk(self._lib.zkp_kzg_fk20_setup(self._h, _ptr(mono), log2_n, _ptr(out), _ptr(out_inf)))
        return out, out_inf

    def kzg_fk20(self, fk20_setup, fk20_setup_inf, coeffs, log2_n, bitrev=False):
        """The KZG proofs of n polynomials at ALL N = 2^log2_n roots of unity (zkp_kzg_fk20_batch): coeffs (n N, 4) in coefficient form,
        canonical; fk20_setup (2N, 12) and fk20_setup_inf (2N,) from kzg_fk20_setup.  -> (proofs (n N, 12), inf (n N,)): proof m of
        polynomial j is [(f_j(tau) - f_j(w^m)) / (tau - w^m)] g1, slot m belonging to w^bitrev(m) with bitrev.  The values are fr_ntt of the
        same coefficients.  Resident torch tensors (all three) stay on the GPU."""
        log2_n, flags = int(log2_n), _lib.NTT_BITREV if bitrev else 0
        if log2_n < 0 or log2_n > 62:
            raise ValueError("log2_n out of range")
        big_n = 1 << log2_n
        if _is_torch(coeffs):
            import torch
            self._t_check(coeffs, 4, "coeffs")
            n_el = coeffs.numel() // 4
            if n_el % big_n:
                raise ValueError("coeffs hold %d elements: no whole number of polynomials of 2^%d" % (n_el, log2_n))
            self._t_check(fk20_setup, 12, "fk20_setup", rows=2 * big_n), self._t_bytes(fk20_setup_inf, 2 * big_n, "fk20_setup_inf")
            proof = torch.empty((n_el, 12), dtype=coeffs.dtype, device=coeffs.device)
            inf = torch.empty(n_el, dtype=torch.uint8, device=coeffs.device)
            self._chk(self._lib.zkp_kzg_fk20_batch_dev(self._h, self._tp(fk20_setup), self._tp(fk20_setup_inf), self._tp(coeffs), n_el >> log2_n, log2_n, flags,
                                                       self._tp(proof), self._tp(inf), self._stream()))
            return proof, inf
        cf = np.ascontiguousarray(coeffs, dtype=np.uint64)
        n_el = cf.size // 4
        if cf.size % 4 or n_el % big_n:
            raise ValueError("coeffs hold %d elements: no whole number of polynomials of 2^%d" % (n_el, log2_n))
        setup = _np(fk20_setup, 12)
        if setup.shape[0] != 2 * big_n:
            raise ValueError("the FK20 setup holds %d points for polynomials of 2^%d" % (setup.shape[0], log2_n))
        sinf = _flags(fk20_setup_inf, 2 * big_n, "kzg_fk20")
        proof, inf = np.empty((n_el, 12), dtype=np.uint64), np.empty(n_el, dtype=np.uint8)
        self._chk(self._lib.zkp_kzg_fk20_batch(self._h, _ptr(setup), _ptr(sinf), _ptr(cf), n_el >> log2_n, log2_n, flags, _ptr(proof), _ptr(inf)))
        return proof, inf

    # ------------------------------------------------------------------ the KZG cell proofs (include/zkp_cells.h)
    @staticmethod
    def _cell_shape(log2_n, log2_l, log2_ext=0):
        log2_n, log2_l, log2_ext = int(log2_n), int(log2_l), int(log2_ext)
        if not (0 <= log2_l <= log2_n <= 62 and log2_ext in (0, 1)):
            raise ValueError("cells: log2_l <= log2_n and log2_ext in (0, 1) expected, got %d, %d, %d" % (log2_l, log2_n, log2_ext))
        return log2_n, log2_l, log2_ext

    def kzg_cells_setup(self, monomial_g1, log2_n, log2_l):
        """(setup (2N, 12), inf (2N,)) for kzg_cells with cells of l = 2^log2_l values, from the monomial setup monomial_g1[k] = [tau^k] g1,
        k < N = 2^log2_n (zkp_kzg_cells_setup): l vectors of 2 N / l points, computed once per setup and cell size.  The points are
        trusted.  A resident torch tensor stays on the GPU."""
        log2_n, log2_l, _ = self._cell_shape(log2_n, log2_l)
        big_n = 1 << log2_n
        if _is_torch(monomial_g1):
            import torch
            self._t_check(monomial_g1, 12, "monomial_g1", rows=big_n)
            out = torch.empty((2 * big_n, 12), dtype=monomial_g1.dtype, device=monomial_g1.device)
            out_inf = torch.empty(2 * big_n, dtype=torch.uint8, device=monomial_g1.device)
            self._chk(self._lib.zkp_kzg_cells_setup_dev(self._h, self._tp(monomial_g1), log2_n, log2_l, self._tp(out), self._tp(out_inf), self._stream()))
            return out, out_inf
        mono = _np(monomial_g1, 12)
        if mono.shape[0] != big_n:
            raise ValueError("the monomial setup holds %d points for polynomials of 2^%d" % (mono.shape[0], log2_n))
        out, out_inf = np.empty((2 * big_n, 12), dtype=np.uint64), np.empty(2 * big_n, dtype=np.uint8)
        self._chk(self._lib.zkp_kzg_cells_setup(self._h, _ptr(mono), log2_n, log2_l, _ptr(out), _ptr(out_inf)))
        return out, out_inf

    def kzg_cells(self, cells_setup, cells_setup_inf, coeffs, log2_n, log2_l, log2_ext=1, bitrev=False):
        """The KZG cell proofs of n polynomials (zkp_kzg_cells_batch): coeffs (n N, 4) in coefficient form, canonical; cells_setup (2N, 12)
        and cells_setup_inf (2N,) from kzg_cells_setup with the same log2_l.  -> (proofs (n M, 12), inf (n M,)), M = 2^log2_ext N / l:
        proof m of polynomial j opens it on the coset w_D^m' H_l, m' = bitrev_M(m) with bitrev.  The cells' values are fr_ntt of the
        coefficients zero-padded to 2^log2_ext N.  Resident torch tensors (all three) stay on the GPU."""
        log2_n, log2_l, log2_ext = self._cell_shape(log2_n, log2_l, log2_ext)
        flags, big_n, log2_m = _lib.NTT_BITREV if bitrev else 0, 1 << log2_n, log2_n - log2_l + log2_ext
        if _is_torch(coeffs):
            import torch
            self._t_check(coeffs, 4, "coeffs")
            n_el = coeffs.numel() // 4
            if n_el % big_n:
                raise ValueError("coeffs hold %d elements: no whole number of polynomials of 2^%d" % (n_el, log2_n))
            n = n_el >> log2_n
            self._t_check(cells_setup, 12, "cells_setup", rows=2 * big_n), self._t_bytes(cells_setup_inf, 2 * big_n, "cells_setup_inf")
            proof = torch.empty((n << log2_m, 12), dtype=coeffs.dtype, device=coeffs.device)
            inf = torch.empty(n << log2_m, dtype=torch.uint8, device=coeffs.device)
            self._chk(self._lib.zkp_kzg_cells_batch_dev(self._h, self._tp(cells_setup), self._tp(cells_setup_inf), self._tp(coeffs), n, log2_n, log2_l, log2_ext,
                                                        flags, self._tp(proof), self._tp(inf), self._stream()))
            return proof, inf
        cf = np.ascontiguousarray(coeffs, dtype=np.uint64)
        n_el = cf.size // 4
        if cf.size % 4 or n_el % big_n:
            raise ValueError("coeffs hold %d elements: no whole number of polynomials of 2^%d" % (n_el, log2_n))
        n = n_el >> log2_n
        setup = _np(cells_setup, 12)
        if setup.shape[0] != 2 * big_n:
            raise ValueError("the cell setup holds %d points for polynomials of 2^%d" % (setup.shape[0], log2_n))
        sinf = _flags(cells_setup_inf, 2 * big_n, "kzg_cells")
        proof, inf = np.empty((n << log2_m, 12), dtype=np.uint64), np.empty(n << log2_m, dtype=np.uint8)
        self._chk(self._lib.zkp_kzg_cells_batch(self._h, _ptr(setup), _ptr(sinf), _ptr(cf), n, log2_n, log2_l, log2_ext, flags, _ptr(proof), _ptr(inf)))
        return proof, inf

    def kzg_cell_verify(self, monomial_g1_l, g2, tau_l_g2, c, cell_index, values, proof, log2_d, log2_l, *, bitrev=False, inf_c=None, inf_proof=None, rand=None,
                        points_checked=False, vk_checked=False):
        """n cells against one setup as ONE check (zkp_kzg_cell_verify_batch): monomial_g1_l (l, 12) = [tau^i] g1, g2 / tau_l_g2 (24,) with
        tau_l_g2 = [tau^l] g2; commitments c and proofs (n, 12), cell_index (n,) 32-bit, values (n l, 4).  True iff the random combination
        holds, every point is valid (unless points_checked / vk_checked), every value is below r, every index below 2^(log2_d - log2_l)
        and no (a_j, b_j) is zero.  rand (n, 2) uint64, by default fresh from os.urandom (rlc_random) - never a seeded generator.  Host
        arrays return a bool; resident torch tensors (all of them) an int32 tensor (1,) without synchronising."""
        log2_d, log2_l = int(log2_d), int(log2_l)
        if not 0 <= log2_l <= log2_d <= 62:
            raise ValueError("cells: 0 <= log2_l <= log2_d expected")
        l = 1 << log2_l
        n = (c.numel() if _is_torch(c) else np.asarray(c).size) // 12
        if n == 0:
            return True
        if rand is None:
            rand = self.rlc_random(n)
        flags = (_lib.NTT_BITREV if bitrev else 0) | (_lib.CELLS_POINTS_CHECKED if points_checked else 0) | (_lib.CELLS_VK_CHECKED if vk_checked else 0)
        if _is_torch(c):
            import torch
            dev = torch.device("cuda", self.device)
            for name, x, w, rows in (("monomial_g1_l", monomial_g1_l, 12, l), ("g2", g2, 24, 1), ("tau_l_g2", tau_l_g2, 24, 1), ("c", c, 12, n),
                                     ("values", values, 4, n * l), ("proof", proof, 12, n)):
                self._t_check(x, w, name, rows=rows)
                if x.numel() != rows * w:
                    raise ValueError("%s holds %d elements, %d expected" % (name, x.numel() // w, rows))
            self._t_check(cell_index, None, "cell_index", rows=n, dtypes=(torch.int32, torch.uint32))
            self._t_bytes(inf_c, n, "inf_c"), self._t_bytes(inf_proof, n, "inf_proof")
            if not _is_torch(rand):
                rand = torch.from_numpy(np.ascontiguousarray(rand, dtype=np.uint64).reshape(-1).view(np.int64)).to(dev)
            self._t_check(rand, 2, "rand", rows=n)
            all_ok = torch.empty(1, dtype=torch.int32, device=dev)
            self._chk(self._lib.zkp_kzg_cell_verify_batch_dev(self._h, self._tp(monomial_g1_l), self._tp(g2), self._tp(tau_l_g2), self._tp(c), self._tp(inf_c),
                                                              self._tp(cell_index), self._tp(values), self._tp(proof), self._tp(inf_proof), n, log2_d, log2_l,
                                                              flags, self._tp(rand), self._tp(all_ok), self._stream()))
            return all_ok
        arrs = {}
        for name, x, w, rows in (("monomial_g1_l", monomial_g1_l, 12, l), ("g2", g2, 24, 1), ("tau_l_g2", tau_l_g2, 24, 1), ("c", c, 12, n),
                                 ("values", values, 4, n * l), ("proof", proof, 12, n), ("rand", rand, 2, n)):
            arrs[name] = _np(x, w)
            if arrs[name].shape[0] != rows:
                raise ValueError("%s holds %d elements, %d expected" % (name, arrs[name].shape[0], rows))
        idx = np.ascontiguousarray(cell_index, dtype=np.uint32).reshape(-1)
        if idx.size != n:
            raise ValueError("cell_index holds %d indices for %d cells" % (idx.size, n))
        ic, ip = _flags(inf_c, n, "inf_c"), _flags(inf_proof, n, "inf_proof")
        res = ctypes.c_int(0)
        self._chk(self._lib.zkp_kzg_cell_verify_batch(self._h, _ptr(arrs["monomial_g1_l"]), _ptr(arrs["g2"]), _ptr(arrs["tau_l_g2"]), _ptr(arrs["c"]), _ptr(ic),
                                                      _ptr(idx), _ptr(arrs["values"]), _ptr(arrs["proof"]), _ptr(ip), n, log2_d, log2_l, flags,
                                                      _ptr(arrs["rand"]), ctypes.byref(res)))
        return bool(res.value)

    # ------------------------------------------------------------------ the cell recovery (include/zkp_recover.h)
    def das_recover(self, values, present, log2_n, log2_l, bitrev=False):
        """Erased blobs back from half their cells (zkp_das_recover_batch): values (n M l, 4), the extended blobs in cell order with
        D = 2 N = 2^(log2_n + 1) points and M = D / l cells of l = 2^log2_l values each - the order of the cells and of the values inside a
        cell follows bitrev exactly as in kzg_cells and kzg_cell_verify -, present (n M,) bytes, non-zero where the cell was received; the
        bytes of a missing cell are never interpreted.  -> (coeffs (n N, 4), ok (n,) int32): blob j in coefficient form, canonical, and
        ok[j] = 1 iff at least M / 2 of its cells are present and consistent with a polynomial of degree below N (too few: a zero row).
        Resident torch tensors (both) stay on the GPU."""
        log2_n, log2_l, _ = self._cell_shape(log2_n, log2_l)
        flags, log2_m = _lib.NTT_BITREV if bitrev else 0, log2_n + 1 - log2_l
        if _is_torch(values):
            import torch
            self._t_check(values, 4, "values")
            n_el = values.numel() // 4
            if n_el % (2 << log2_n):
                raise ValueError("values hold %d elements: no whole number of extended blobs of 2^%d" % (n_el, log2_n + 1))
            n = n_el >> (log2_n + 1)
            if present is None:
                raise ValueError("das_recover: present is required")
            self._t_bytes(present, n << log2_m, "present")
            coeffs = torch.empty((n << log2_n, 4), dtype=values.dtype, device=values.device)
            ok = torch.empty(n, dtype=torch.int32, device=values.device)
            self._chk(self._lib.zkp_das_recover_batch_dev(self._h, self._tp(values), self._tp(present), n, log2_n, log2_l, flags, self._tp(coeffs), self._tp(ok),
                                                          self._stream()))
            return coeffs, ok
        v = np.ascontiguousarray(values, dtype=np.uint64)
        n_el = v.size // 4
        if v.size % 4 or n_el % (2 << log2_n):
            raise ValueError("values hold %d elements: no whole number of extended blobs of 2^%d" % (n_el, log2_n + 1))
        n = n_el >> (log2_n + 1)
        if present is None:
            raise ValueError("das_recover: present is required")
        pr = _flags(present, n << log2_m, "das_recover")
        coeffs, ok = np.empty((n << log2_n, 4), dtype=np.uint64), np.empty(n, dtype=np.int32)
        self._chk(self._lib.zkp_das_recover_batch(self._h, _ptr(v), _ptr(pr), n, log2_n, log2_l, flags, _ptr(coeffs), _ptr(ok)))
        return coeffs, ok

    # ------------------------------------------------------------------ hash-to-G2 and BLS signatures (include/zkp_bls.h)
    @staticmethod
    def pack_messages(msgs):
        """a list of bytes objects -> (buffer uint8, offsets uint64 (n + 1,)): the message layout of the hash and verify calls"""
        offsets = np.zeros(len(msgs) + 1, dtype=np.uint64)
        if len(msgs):
            offsets[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
        return np.frombuffer(b"".join(bytes(x) for x in msgs), dtype=np.uint8), offsets

    def _msgs_np(self, msgs, offsets, dst):
        if offsets is None:
            msgs, offsets = self.pack_messages(msgs)
        buf = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(-1)
        off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if off.size < 1:
            raise ValueError("offsets: n + 1 values, at least one")
        if off.size > 1 and int(off.max()) > buf.size:
            raise ValueError("offsets reach byte %d of a buffer of %d" % (int(off.max()), buf.size))
        d = np.frombuffer(bytes(dst), dtype=np.uint8)
        return buf, off, off.size - 1, d

    def _msgs_t(self, msgs, offsets, dst):
        import torch
        u8 = (torch.uint8,)
        self._t_check(offsets, None, "offsets", rows=1)
        if msgs is not None:
            self._t_check(msgs, None, "msgs", dtypes=u8)
        if not _is_torch(dst):
            dst = torch.frombuffer(bytearray(bytes(dst)), dtype=torch.uint8).to(offsets.device)
        self._t_check(dst, None, "dst", dtypes=u8)
        return msgs, offsets, offsets.numel() - 1, dst

    def fp_from_wide_be(self, data):
        """64 big-endian bytes per element -> canonical Fp (n, 6): OS2IP mod p (zkp_fp_from_wide_be_batch)"""
        if _is_torch(data):
            import torch
            self._t_check(data, 64, "data", dtypes=(torch.uint8,))
            n = data.numel() // 64
            out = torch.empty((n, 6), dtype=torch.int64, device=data.device)
            self._chk(self._lib.zkp_fp_from_wide_be_batch_dev(self._h, self._tp(data), n, self._tp(out), self._stream()))
            return out
        b = _np(data, 64, np.uint8)
        out = np.empty((b.shape[0], 6), dtype=np.uint64)
        self._chk(self._lib.zkp_fp_from_wide_be_batch(self._h, _ptr(b), b.shape[0], _ptr(out)))
        return out

    def hash_to_field_g2(self, msgs, dst, offsets=None):
        """messages -> (u0, u1) of RFC 9380 hash_to_field for G2, (n, 24) words (zkp_hash_to_field_g2_batch).  msgs: a list of bytes, or
        a byte buffer with offsets (n + 1,); torch tensors (buffer uint8, offsets int64, dst bytes or a uint8 tensor) stay on the GPU."""
        if _is_torch(offsets):
            import torch
            msgs, offsets, n, dst = self._msgs_t(msgs, offsets, dst)
            out = torch.empty((n, 24), dtype=torch.int64, device=offsets.device)
            self._chk(self._lib.zkp_hash_to_field_g2_batch_dev(self._h, self._tp(msgs), self._tp(offsets), n, self._tp(dst), dst.numel(), self._tp(out),
                                                               self._stream()))
            return out
        buf, off, n, d = self._msgs_np(msgs, offsets, dst)
        out = np.empty((n, 24), dtype=np.uint64)
        self._chk(self._lib.zkp_hash_to_field_g2_batch(self._h, _ptr(buf), _ptr(off), n, _ptr(d), d.size, _ptr(out)))
        return out

    def g2_map_from_fields(self, u):
        """u (n, 24): two Fp2 elements per point -> clear_cofactor(iso(sswu(u0)) + iso(sswu(u1))): (points (n, 24), inf (n,))"""
        if _is_torch(u):
            import torch
            self._t_check(u, 24, "u")
            n = u.numel() // 24
            out, oi = torch.empty((n, 24), dtype=u.dtype, device=u.device), torch.empty(n, dtype=torch.uint8, device=u.device)
            self._chk(self._lib.zkp_g2_map_from_fields_batch_dev(self._h, self._tp(u), n, self._tp(out), self._tp(oi), self._stream()))
            return out, oi
        u = _np(u, 24)
        out, oi = np.empty((u.shape[0], 24), dtype=np.uint64), np.empty(u.shape[0], dtype=np.uint8)
        self._chk(self._lib.zkp_g2_map_from_fields_batch(self._h, _ptr(u), u.shape[0], _ptr(out), _ptr(oi)))
        return out, oi

    def g2_clear_cofactor(self, pts, inf=None):
        """[h_eff] P for any points of E2 (zkp_g2_clear_cofactor_batch): (points (n, 24), inf (n,))"""
        if _is_torch(pts):
            import torch
            self._t_check(pts, 24, "pts")
            n = pts.numel() // 24
            self._t_bytes(inf, n, "inf")
            out, oi = torch.empty((n, 24), dtype=pts.dtype, device=pts.device), torch.empty(n, dtype=torch.uint8, device=pts.device)
            self._chk(self._lib.zkp_g2_clear_cofactor_batch_dev(self._h, self._tp(pts), self._tp(inf), n, self._tp(out), self._tp(oi), self._stream()))
            return out, oi
        pts = _np(pts, 24)
        n = pts.shape[0]
        i = _flags(inf, n, "inf")
        out, oi = np.empty((n, 24), dtype=np.uint64), np.empty(n, dtype=np.uint8)
        self._chk(self._lib.zkp_g2_clear_cofactor_batch(self._h, _ptr(pts), _ptr(i), n, _ptr(out), _ptr(oi)))
        return out, oi

    def hash_to_g2(self, msgs, dst, offsets=None):
        """messages -> points of G2 (RFC 9380 BLS12381G2_XMD:SHA-256_SSWU_RO_; zkp_hash_to_g2_batch): (points (n, 24), inf (n,));
        the arguments of hash_to_field_g2"""
        if _is_torch(offsets):
            import torch
            msgs, offsets, n, dst = self._msgs_t(msgs, offsets, dst)
            out, oi = torch.empty((n, 24), dtype=torch.int64, device=offsets.device), torch.empty(n, dtype=torch.uint8, device=offsets.device)
            self._chk(self._lib.zkp_hash_to_g2_batch_dev(self._h, self._tp(msgs), self._tp(offsets), n, self._tp(dst), dst.numel(), self._tp(out), self._tp(oi),
                                                         self._stream()))
            return out, oi
        buf, off, n, d = self._msgs_np(msgs, offsets, dst)
        out, oi = np.empty((n, 24), dtype=np.uint64), np.empty(n, dtype=np.uint8)
        self._chk(self._lib.zkp_hash_to_g2_batch(self._h, _ptr(buf), _ptr(off), n, _ptr(d), d.size, _ptr(out), _ptr(oi)))
        return out, oi

    def bls_verify(self, pk, msgs, sig, dst, offsets=None, inf_pk=None, inf_sig=None, rand=None, points_checked=False, all_ok=None):
        """n BLS signatures (public keys in G1, signatures in G2) verified as ONE pairing product (zkp_bls_verify_batch): True iff
        prod_i e([r_i] pk_i, H(m_i)) e(-g1, sum_i [r_i] sig_i) == 1, every pk and sig is valid (unless points_checked), no pk is the
        identity and no (a_i, b_i) of rand is zero.  rand (n, 2) uint64, by default fresh from os.urandom (rlc_random).  Host arrays
        return a bool; resident torch tensors fill and return all_ok (int32 (1,)) without synchronising."""
        flags = _lib.BLS_POINTS_CHECKED if points_checked else 0
        if _is_torch(pk):
            import torch
            self._t_check(pk, 12, "pk"), self._t_check(sig, 24, "sig")
            msgs, offsets, n, dst = self._msgs_t(msgs, offsets, dst)
            if pk.numel() // 12 != n or sig.numel() // 24 != n:
                raise ValueError("%d messages, %d public keys, %d signatures" % (n, pk.numel() // 12, sig.numel() // 24))
            self._t_bytes(inf_pk, n, "inf_pk"), self._t_bytes(inf_sig, n, "inf_sig")
            if rand is None:
                rand = torch.from_numpy(self.rlc_random(n).view(np.int64)).to(pk.device)
            self._t_check(rand, 2, "rand", rows=n)
            if all_ok is None:
                all_ok = torch.empty(1, dtype=torch.int32, device=pk.device)
            self._t_check(all_ok, None, "all_ok", rows=1, dtypes=(torch.int32,))
            self._chk(self._lib.zkp_bls_verify_batch_dev(self._h, self._tp(pk), self._tp(inf_pk), self._tp(msgs), self._tp(offsets), self._tp(dst), dst.numel(),
                                                         self._tp(sig), self._tp(inf_sig), n, self._tp(rand), flags, self._tp(all_ok), self._stream()))
            return all_ok
        buf, off, n, d = self._msgs_np(msgs, offsets, dst)
        pk, sig = _np(pk, 12), _np(sig, 24)
        if pk.shape[0] != n or sig.shape[0] != n:
            raise ValueError("%d messages, %d public keys, %d signatures" % (n, pk.shape[0], sig.shape[0]))
        ip, isg = _flags(inf_pk, n, "inf_pk"), _flags(inf_sig, n, "inf_sig")
        r = self.rlc_random(n) if rand is None else _np(rand, 2)
        if r.shape[0] != n:
            raise ValueError("rand holds %d pairs for %d signatures" % (r.shape[0], n))
        ok = ctypes.c_int(0)
        self._chk(self._lib.zkp_bls_verify_batch(self._h, _ptr(pk), _ptr(ip), _ptr(buf), _ptr(off), _ptr(d), d.size, _ptr(sig), _ptr(isg), n, _ptr(r), flags,
                                                 ctypes.byref(ok)))
        return bool(ok.value)

    # ------------------------------------------------------------------ hash-to-G1 and min-sig BLS signatures (include/zkp_bls_minsig.h)
    def hash_to_field_g1(self, msgs, dst, offsets=None):
        """messages -> (u0, u1) of RFC 9380 hash_to_field for G1, (n, 12) words (zkp_hash_to_field_g1_batch); the arguments of
        hash_to_field_g2"""
        if _is_torch(offsets):
            import torch
            msgs, offsets, n, dst = self._msgs_t(msgs, offsets, dst)
            out = torch.empty((n, 12), dtype=torch.int64, device=offsets.device)
            self._chk(self._lib.zkp_hash_to_field_g1_batch_dev(self._h, self._tp(msgs), self._tp(offsets), n, self._tp(dst), dst.numel(), self._tp(out),
                                                               self._stream()))
            return out
        buf, off, n, d = self._msgs_np(msgs, offsets, dst)
        out = np.empty((n, 12), dtype=np.uint64)
        self._chk(self._lib.zkp_hash_to_field_g1_batch(self._h, _ptr(buf), _ptr(off), n, _ptr(d), d.size, _ptr(out)))
        return out

    def g1_map_from_fields(self, u):
        """u (n, 12): two Fp elements per point -> clear_cofactor(iso(sswu(u0)) + iso(sswu(u1))): (points (n, 12), inf (n,))"""
        if _is_torch(u):
            import torch
            self._t_check(u, 12, "u")
            n = u.numel() // 12
            out, oi = torch.empty((n, 12), dtype=u.dtype, device=u.device), torch.empty(n, dtype=torch.uint8, device=u.device)
            self._chk(self._lib.zkp_g1_map_from_fields_batch_dev(self._h, self._tp(u), n, self._tp(out), self._tp(oi), self._stream()))
            return out, oi
        u = _np(u, 12)
        out, oi = np.empty((u.shape[0], 12), dtype=np.uint64), np.empty(u.shape[0], dtype=np.uint8)
        self._chk(self._lib.zkp_g1_map_from_fields_batch(self._h, _ptr(u), u.shape[0], _ptr(out), _ptr(oi)))
        return out, oi

    def g1_clear_cofactor(self, pts, inf=None):
        """[1 - x] P for any points of E: y^2 = x^3 + 4 (zkp_g1_clear_cofactor_batch): (points (n, 12), inf (n,))"""
        if _is_torch(pts):
            import torch
            self._t_check(pts, 12, "pts")
            n = pts.numel() // 12
            self._t_bytes(inf, n, "inf")
            out, oi = torch.empty((n, 12), dtype=pts.dtype, device=pts.device), torch.empty(n, dtype=torch.uint8, device=pts.device)
            self._chk(self._lib.zkp_g1_clear_cofactor_batch_dev(self._h, self._tp(pts), self._tp(inf), n, self._tp(out), self._tp(oi), self._stream()))
            return out, oi
        pts = _np(pts, 12)
        n = pts.shape[0]
        i = _flags(inf, n, "inf")
        out, oi = np.empty((n, 12), dtype=np.uint64), np.empty(n, dtype=np.uint8)
        self._chk(self._lib.zkp_g1_clear_cofactor_batch(self._h, _ptr(pts), _ptr(i), n, _ptr(out), _ptr(oi)))
        return out, oi

    def hash_to_g1(self, msgs, dst, offsets=None):
        """messages -> points of G1 (RFC 9380 BLS12381G1_XMD:SHA-256_SSWU_RO_; zkp_hash_to_g1_batch): (points (n, 12), inf (n,)); the
        arguments of hash_to_field_g2"""
        if _is_torch(offsets):
            import torch
            msgs, offsets, n, dst = self._msgs_t(msgs, offsets, dst)
            out, oi = torch.empty((n, 12), dtype=torch.int64, device=offsets.device), torch.empty(n, dtype=torch.uint8, device=offsets.device)
            self._chk(self._lib.zkp_hash_to_g1_batch_dev(self._h, self._tp(msgs), self._tp(offsets), n, self._tp(dst), dst.numel(), self._tp(out), self._tp(oi),
                                                         self._stream()))
            return out, oi
        buf, off, n, d = self._msgs_np(msgs, offsets, dst)
        out, oi = np.empty((n, 12), dtype=np.uint64), np.empty(n, dtype=np.uint8)
        self._chk(self._lib.zkp_hash_to_g1_batch(self._h, _ptr(buf), _ptr(off), n, _ptr(d), d.size, _ptr(out), _ptr(oi)))
        return out, oi

    def bls_minsig_verify(self, pk, msgs, sig, dst, offsets=None, inf_pk=None, inf_sig=None, rand=None, points_checked=False, all_ok=None):
        """n BLS signatures of the minimal-signature-size layout (public keys in G2 (n, 24), signatures in G1 (n, 12)) verified as ONE
        pairing product (zkp_bls_minsig_verify_batch): True iff prod_i e([r_i] H(m_i), pk_i) e(sum_i [r_i] sig_i, -g2) == 1, every pk
        and sig is valid (unless points_checked), no pk is the identity and no (a_i, b_i) of rand is zero.  The arguments and the
        return value of bls_verify."""
        flags = _lib.BLS_POINTS_CHECKED if points_checked else 0
        if _is_torch(pk):
            import torch
            self._t_check(pk, 24, "pk"), self._t_check(sig, 12, "sig")
            msgs, offsets, n, dst = self._msgs_t(msgs, offsets, dst)
            if pk.numel() // 24 != n or sig.numel() // 12 != n:
                raise ValueError("%d messages, %d public keys, %d signatures" % (n, pk.numel() // 24, sig.numel() // 12))
            self._t_bytes(inf_pk, n, "inf_pk"), self._t_bytes(inf_sig, n, "inf_sig")
            if rand is None:
                rand = torch.from_numpy(self.rlc_random(n).view(np.int64)).to(pk.device)
            self._t_check(rand, 2, "rand", rows=n)
            if all_ok is None:
                all_ok = torch.empty(1, dtype=torch.int32, device=pk.device)
            self._t_check(all_ok, None, "all_ok", rows=1, dtypes=(torch.int32,))
            self._chk(self._lib.zkp_bls_minsig_verify_batch_dev(self._h, self._tp(pk), self._tp(inf_pk), self._tp(msgs), self._tp(offsets), self._tp(dst),
                                                                dst.numel(), self._tp(sig), self._tp(inf_sig), n, self._tp(rand), flags, self._tp(all_ok),
                                                                self._stream()))
            return all_ok
        buf, off, n, d = self._msgs_np(msgs, offsets, dst)
        pk, sig = _np(pk, 24), _np(sig, 12)
        if pk.shape[0] != n or sig.shape[0] != n:
            raise ValueError("%d messages, %d public keys, %d signatures" % (n, pk.shape[0], sig.shape[0]))
        ip, isg = _flags(inf_pk, n, "inf_pk"), _flags(inf_sig, n, "inf_sig")
        r = self.rlc_random(n) if rand is None else _np(rand, 2)
        if r.shape[0] != n:
            raise ValueError("rand holds %d pairs for %d signatures" % (r.shape[0], n))
        ok = ctypes.c_int(0)
        self._chk(self._lib.zkp_bls_minsig_verify_batch(self._h, _ptr(pk), _ptr(ip), _ptr(buf), _ptr(off), _ptr(d), d.size, _ptr(sig), _ptr(isg), n, _ptr(r),
                                                        flags, ctypes.byref(ok)))
        return bool(ok.value)

    def bls_minsig_verify_samekey(self, pk, msgs, sig, dst, offsets=None, inf_sig=None, rand=None, points_checked=False, all_ok=None):
        """bls_minsig_verify when ONE key pk (24 words) signed every message (zkp_bls_minsig_verify_samekey_batch): two G1 sums, two
        Miller loops.  The same answer as bls_minsig_verify with the key repeated and the same rand."""
        flags = _lib.BLS_POINTS_CHECKED if points_checked else 0
        if _is_torch(pk):
            import torch
            self._t_check(pk, 24, "pk", rows=1), self._t_check(sig, 12, "sig")
            msgs, offsets, n, dst = self._msgs_t(msgs, offsets, dst)
            if sig.numel() // 12 != n:
                raise ValueError("%d messages, %d signatures" % (n, sig.numel() // 12))
            self._t_bytes(inf_sig, n, "inf_sig")
            if rand is None:
                rand = torch.from_numpy(self.rlc_random(n).view(np.int64)).to(pk.device)
            self._t_check(rand, 2, "rand", rows=n)
            if all_ok is None:
                all_ok = torch.empty(1, dtype=torch.int32, device=pk.device)
            self._t_check(all_ok, None, "all_ok", rows=1, dtypes=(torch.int32,))
            self._chk(self._lib.zkp_bls_minsig_verify_samekey_batch_dev(self._h, self._tp(pk), self._tp(msgs), self._tp(offsets), self._tp(dst), dst.numel(),
                                                                        self._tp(sig), self._tp(inf_sig), n, self._tp(rand), flags, self._tp(all_ok),
                                                                        self._stream()))
            return all_ok
        buf, off, n, d = self._msgs_np(msgs, offsets, dst)
        pk, sig = _np(pk, 24), _np(sig, 12)
        if pk.shape[0] != 1 or sig.shape[0] != n:
            raise ValueError("%d messages, %d public keys (one wanted), %d signatures" % (n, pk.shape[0], sig.shape[0]))
        isg = _flags(inf_sig, n, "inf_sig")
        r = self.rlc_random(n) if rand is None else _np(rand, 2)
        if r.shape[0] != n:
            raise ValueError("rand holds %d pairs for %d signatures" % (r.shape[0], n))
        ok = ctypes.c_int(0)
        self._chk(self._lib.zkp_bls_minsig_verify_samekey_batch(self._h, _ptr(pk), _ptr(buf), _ptr(off), _ptr(d), d.size, _ptr(sig), _ptr(isg), n, _ptr(r),
                                                                flags, ctypes.byref(ok)))
        return bool(ok.value)

    # ------------------------------------------------------------------ committee aggregation (include/zkp_bls_agg.h)
    @staticmethod
    def _entries_np(idx, seg_off):
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        seg_off = np.ascontiguousarray(seg_off, dtype=np.uint64).reshape(-1)
        if seg_off.size < 1:
            raise ValueError("seg_off: n_seg + 1 values, at least one")
        return idx, seg_off

    def _entries_t(self, table, idx, seg_off, cols=12):
        import torch
        self._t_check(table, cols, "table")
        self._t_check(idx, None, "idx", dtypes=(torch.int32, torch.uint32))
        self._t_check(seg_off, None, "seg_off", rows=1)
        return table.numel() // cols, idx.numel(), seg_off.numel() - 1

    def g1_segment_sum(self, table, idx, seg_off):
        """out[j] = sum of (+/-) table[idx[e] & 0x7fffffff] over e in [seg_off[j], seg_off[j + 1]) (bit 31 of idx[e]: subtract;
        zkp_g1_segment_sum_batch): (points (n_seg, 12), inf (n_seg,), status (n_seg,)).  table (n_table, 12) finite G1 points, idx uint32,
        seg_off (n_seg + 1,) uint64.  Host arrays with malformed offsets or a row beyond the table raise; resident torch tensors (idx int32,
        seg_off int64) stay on the GPU, where such a segment is the identity with status 1."""
        if _is_torch(table):
            import torch
            n_table, n_idx, n_seg = self._entries_t(table, idx, seg_off)
            out = torch.empty((n_seg, 12), dtype=table.dtype, device=table.device)
            oi, st = torch.empty(n_seg, dtype=torch.uint8, device=table.device), torch.empty(n_seg, dtype=torch.uint8, device=table.device)
            self._chk(self._lib.zkp_g1_segment_sum_batch_dev(self._h, self._tp(table), n_table, self._tp(idx), n_idx, self._tp(seg_off), n_seg, self._tp(out),
                                                             self._tp(oi), self._tp(st), self._stream()))
            return out, oi, st
        table = _np(table, 12)
        idx, seg_off = self._entries_np(idx, seg_off)
        n_seg = seg_off.size - 1
        out, oi, st = np.empty((n_seg, 12), dtype=np.uint64), np.empty(n_seg, dtype=np.uint8), np.empty(n_seg, dtype=np.uint8)
        self._chk(self._lib.zkp_g1_segment_sum_batch(self._h, _ptr(table), table.shape[0], _ptr(idx), idx.size, _ptr(seg_off), n_seg, _ptr(out), _ptr(oi),
                                                     _ptr(st)))
        return out, oi, st

    def bls_fast_aggregate_verify(self, table, idx, seg_off, msgs, sig, dst, offsets=None, inf_sig=None, rand=None, points_checked=False, all_ok=None):
        """n aggregate signatures, each by the committee idx[seg_off[i] .. seg_off[i + 1]) of the key table on message i
        (zkp_bls_fast_aggregate_verify_batch): True iff bls_verify holds on the committees' key sums, no committee is empty and no row
        lies beyond the table.  The arguments of g1_segment_sum and bls_verify; host arrays return a bool, resident torch tensors fill and
        return all_ok (int32 (1,)) without synchronising."""
        flags = _lib.BLS_POINTS_CHECKED if points_checked else 0
        if _is_torch(table):
            import torch
            n_table, n_idx, n = self._entries_t(table, idx, seg_off)
            self._t_check(sig, 24, "sig")
            msgs, offsets, n_msg, dst = self._msgs_t(msgs, offsets, dst)
            if n_msg != n or sig.numel() // 24 != n:
                raise ValueError("%d committees, %d messages, %d signatures" % (n, n_msg, sig.numel() // 24))
            self._t_bytes(inf_sig, n, "inf_sig")
            if rand is None:
                rand = torch.from_numpy(self.rlc_random(n).view(np.int64)).to(table.device)
            self._t_check(rand, 2, "rand", rows=n)
            if all_ok is None:
                all_ok = torch.empty(1, dtype=torch.int32, device=table.device)
            self._t_check(all_ok, None, "all_ok", rows=1, dtypes=(torch.int32,))
            self._chk(self._lib.zkp_bls_fast_aggregate_verify_batch_dev(self._h, self._tp(table), n_table, self._tp(idx), n_idx, self._tp(seg_off), self._tp(msgs),
                                                                        self._tp(offsets), self._tp(dst), dst.numel(), self._tp(sig), self._tp(inf_sig), n,
                                                                        self._tp(rand), flags, self._tp(all_ok), self._stream()))
            return all_ok
        table, sig = _np(table, 12), _np(sig, 24)
        idx, seg_off = self._entries_np(idx, seg_off)
        buf, off, n, d = self._msgs_np(msgs, offsets, dst)
        if seg_off.size - 1 != n or sig.shape[0] != n:
            raise ValueError("%d committees, %d messages, %d signatures" % (seg_off.size - 1, n, sig.shape[0]))
        isg = _flags(inf_sig, n, "inf_sig")
        r = self.rlc_random(n) if rand is None else _np(rand, 2)
        if r.shape[0] != n:
            raise ValueError("rand holds %d pairs for %d signatures" % (r.shape[0], n))
        ok = ctypes.c_int(0)
        self._chk(self._lib.zkp_bls_fast_aggregate_verify_batch(self._h, _ptr(table), table.shape[0], _ptr(idx), idx.size, _ptr(seg_off), _ptr(buf), _ptr(off),
                                                                _ptr(d), d.size, _ptr(sig), _ptr(isg), n, _ptr(r), flags, ctypes.byref(ok)))
        return bool(ok.value)

    # ------------------------------------------------------------------ G2 aggregation and AggregateVerify (include/zkp_bls_agg_g2.h)
    def g2_segment_sum(self, table, idx, seg_off):
        """g1_segment_sum over a table (n_table, 24) of finite G2 points (zkp_g2_segment_sum_batch): (points (n_seg, 24), inf (n_seg,),
        status (n_seg,)) - the aggregate of signatures in the min-pk layout, of public keys in the min-sig layout.  The entries, the
        refusals and the two flavours are those of g1_segment_sum."""
        if _is_torch(table):
            import torch
            n_table, n_idx, n_seg = self._entries_t(table, idx, seg_off, 24)
            out = torch.empty((n_seg, 24), dtype=table.dtype, device=table.device)
            oi, st = torch.empty(n_seg, dtype=torch.uint8, device=table.device), torch.empty(n_seg, dtype=torch.uint8, device=table.device)
            self._chk(self._lib.zkp_g2_segment_sum_batch_dev(self._h, self._tp(table), n_table, self._tp(idx), n_idx, self._tp(seg_off), n_seg, self._tp(out),
                                                             self._tp(oi), self._tp(st), self._stream()))
            return out, oi, st
        table = _np(table, 24)
        idx, seg_off = self._entries_np(idx, seg_off)
        n_seg = seg_off.size - 1
        out, oi, st = np.empty((n_seg, 24), dtype=np.uint64), np.empty(n_seg, dtype=np.uint8), np.empty(n_seg, dtype=np.uint8)
        self._chk(self._lib.zkp_g2_segment_sum_batch(self._h, _ptr(table), table.shape[0], _ptr(idx), idx.size, _ptr(seg_off), n_seg, _ptr(out), _ptr(oi),
                                                     _ptr(st)))
        return out, oi, st

    def bls_minsig_fast_aggregate_verify(self, table, idx, seg_off, msgs, sig, dst, offsets=None, inf_sig=None, rand=None, points_checked=False,
                                         all_ok=None):
        """bls_fast_aggregate_verify in the minimal-signature-size layout (zkp_bls_minsig_fast_aggregate_verify_batch): the key table is
        (n_table, 24) in G2, the aggregate signatures (n, 12) in G1; True iff bls_minsig_verify holds on the committees' key sums, no
        committee is empty and no row lies beyond the table.  The arguments and the return value of bls_fast_aggregate_verify."""
        flags = _lib.BLS_POINTS_CHECKED if points_checked else 0
        if _is_torch(table):
            import torch
            n_table, n_idx, n = self._entries_t(table, idx, seg_off, 24)
            self._t_check(sig, 12, "sig")
            msgs, offsets, n_msg, dst = self._msgs_t(msgs, offsets, dst)
            if n_msg != n or sig.numel() // 12 != n:
                raise ValueError("%d committees, %d messages, %d signatures" % (n, n_msg, sig.numel() // 12))
            self._t_bytes(inf_sig, n, "inf_sig")
            if rand is None:
                rand = torch.from_numpy(self.rlc_random(n).view(np.int64)).to(table.device)
            self._t_check(rand, 2, "rand", rows=n)
            if all_ok is None:
                all_ok = torch.empty(1, dtype=torch.int32, device=table.device)
            self._t_check(all_ok, None, "all_ok", rows=1, dtypes=(torch.int32,))
            self._chk(self._lib.zkp_bls_minsig_fast_aggregate_verify_batch_dev(self._h, self._tp(table), n_table, self._tp(idx), n_idx, self._tp(seg_off),
                                                                               self._tp(msgs), self._tp(offsets), self._tp(dst), dst.numel(), self._tp(sig),
                                                                               self._tp(inf_sig), n, self._tp(rand), flags, self._tp(all_ok), self._stream()))
            return all_ok
        table, sig = _np(table, 24), _np(sig, 12)
        idx, seg_off = self._entries_np(idx, seg_off)
        buf, off, n, d = self._msgs_np(msgs, offsets, dst)
        if seg_off.size - 1 != n or sig.shape[0] != n:
            raise ValueError("%d committees, %d messages, %d signatures" % (seg_off.size - 1, n, sig.shape[0]))
        isg = _flags(inf_sig, n, "inf_sig")
        r = self.rlc_random(n) if rand is None else _np(rand, 2)
        if r.shape[0] != n:
            raise ValueError("rand holds %d pairs for %d signatures" % (r.shape[0], n))
        ok = ctypes.c_int(0)
        self._chk(self._lib.zkp_bls_minsig_fast_aggregate_verify_batch(self._h, _ptr(table), table.shape[0], _ptr(idx), idx.size, _ptr(seg_off), _ptr(buf),
                                                                       _ptr(off), _ptr(d), d.size, _ptr(sig), _ptr(isg), n, _ptr(r), flags, ctypes.byref(ok)))
        return bool(ok.value)

    def bls_aggregate_verify(self, pk, msgs, seg_off, sig, dst, offsets=None, inf_pk=None, inf_sig=None, rand=None, points_checked=False, all_ok=None):
        """n aggregate signatures (n, 24), signature j over the pairs (pk_i, m_i) for i in [seg_off[j], seg_off[j + 1]) of n_msg public keys
        (n_msg, 12) and messages (zkp_bls_aggregate_verify_batch): True iff bls_verify holds with signature j filed under the first message
        of its segment, the identity under the others and rand row j on all of them, the offsets are well formed and no segment is empty.
        inf_pk (n_msg,), inf_sig (n,), rand (n, 2).  Messages of one segment are not tested for distinctness.  Host arrays return a bool
        (malformed seg_off raises); resident torch tensors (seg_off int64) fill and return all_ok (int32 (1,)) without synchronising."""
        flags = _lib.BLS_POINTS_CHECKED if points_checked else 0
        if _is_torch(pk):
            import torch
            self._t_check(pk, 12, "pk"), self._t_check(sig, 24, "sig")
            self._t_check(seg_off, None, "seg_off", rows=1)
            msgs, offsets, n_msg, dst = self._msgs_t(msgs, offsets, dst)
            n = seg_off.numel() - 1
            if pk.numel() // 12 != n_msg or sig.numel() // 24 != n:
                raise ValueError("%d messages, %d public keys; %d segments, %d signatures" % (n_msg, pk.numel() // 12, n, sig.numel() // 24))
            self._t_bytes(inf_pk, n_msg, "inf_pk"), self._t_bytes(inf_sig, n, "inf_sig")
            if rand is None:
                rand = torch.from_numpy(self.rlc_random(n).view(np.int64)).to(pk.device)
            self._t_check(rand, 2, "rand", rows=n)
            if all_ok is None:
                all_ok = torch.empty(1, dtype=torch.int32, device=pk.device)
            self._t_check(all_ok, None, "all_ok", rows=1, dtypes=(torch.int32,))
            self._chk(self._lib.zkp_bls_aggregate_verify_batch_dev(self._h, self._tp(pk), self._tp(inf_pk), self._tp(msgs), self._tp(offsets), n_msg,
                                                                   self._tp(seg_off), self._tp(dst), dst.numel(), self._tp(sig), self._tp(inf_sig), n,
                                                                   self._tp(rand), flags, self._tp(all_ok), self._stream()))
            return all_ok
        buf, off, n_msg, d = self._msgs_np(msgs, offsets, dst)
        pk, sig = _np(pk, 12), _np(sig, 24)
        seg_off = self._offsets_np(seg_off, "seg_off")
        n = seg_off.size - 1
        if pk.shape[0] != n_msg or sig.shape[0] != n:
            raise ValueError("%d messages, %d public keys; %d segments, %d signatures" % (n_msg, pk.shape[0], n, sig.shape[0]))
        ip, isg = _flags(inf_pk, n_msg, "inf_pk"), _flags(inf_sig, n, "inf_sig")
        r = self.rlc_random(n) if rand is None else _np(rand, 2)
        if r.shape[0] != n:
            raise ValueError("rand holds %d pairs for %d signatures" % (r.shape[0], n))
        ok = ctypes.c_int(0)
        self._chk(self._lib.zkp_bls_aggregate_verify_batch(self._h, _ptr(pk), _ptr(ip), _ptr(buf), _ptr(off), n_msg, _ptr(seg_off), _ptr(d), d.size, _ptr(sig),
                                                           _ptr(isg), n, _ptr(r), flags, ctypes.byref(ok)))
        return bool(ok.value)

    # ------------------------------------------------------------------ verification grouped by message (include/zkp_bls_grouped.h)
    @staticmethod
    def _offsets_np(off, name):
        off = np.ascontiguousarray(off, dtype=np.uint64).reshape(-1)
        if off.size < 1:
            raise ValueError("%s: count + 1 values, at least one" % name)
        return off

    def g1_scaled_segment_sum(self, pts, rand, seg_off, inf=None):
        """out[g] = sum of [a_i + b_i z^2] pts[i] over i in [seg_off[g], seg_off[g + 1]) with (a_i, b_i) = rand[i]
        (zkp_g1_scaled_segment_sum_batch): (points (n_seg, 12), inf (n_seg,), status (n_seg,)).  pts (n, 12) G1 points, rand (n, 2) uint64,
        seg_off (n_seg + 1,) uint64.  Host arrays with malformed offsets raise; resident torch tensors (int64) stay on the GPU, where a
        malformed call gives identities with status 1."""
        if _is_torch(pts):
            import torch
            self._t_check(pts, 12, "pts")
            n = pts.numel() // 12
            self._t_check(rand, 2, "rand", rows=n)
            self._t_check(seg_off, None, "seg_off", rows=1)
            self._t_bytes(inf, n, "inf")
            n_seg = seg_off.numel() - 1
            out = torch.empty((n_seg, 12), dtype=pts.dtype, device=pts.device)
            oi, st = torch.empty(n_seg, dtype=torch.uint8, device=pts.device), torch.empty(n_seg, dtype=torch.uint8, device=pts.device)
            self._chk(self._lib.zkp_g1_scaled_segment_sum_batch_dev(self._h, self._tp(pts), self._tp(inf), self._tp(rand), n, self._tp(seg_off), n_seg,
                                                                    self._tp(out), self._tp(oi), self._tp(st), self._stream()))
            return out, oi, st
        pts, r = _np(pts, 12), _np(rand, 2)
        n = pts.shape[0]
        if r.shape[0] != n:
            raise ValueError("rand holds %d pairs for %d points" % (r.shape[0], n))
        seg_off = self._offsets_np(seg_off, "seg_off")
        i = _flags(inf, n, "inf")
        n_seg = seg_off.size - 1
        out, oi, st = np.empty((n_seg, 12), dtype=np.uint64), np.empty(n_seg, dtype=np.uint8), np.empty(n_seg, dtype=np.uint8)
        self._chk(self._lib.zkp_g1_scaled_segment_sum_batch(self._h, _ptr(pts), _ptr(i), _ptr(r), n, _ptr(seg_off), n_seg, _ptr(out), _ptr(oi), _ptr(st)))
        return out, oi, st

    def bls_verify_grouped(self, pk, grp_off, msgs, sig, dst, offsets=None, inf_pk=None, inf_sig=None, rand=None, points_checked=False, all_ok=None):
        """n BLS signatures ORDERED BY MESSAGE over m distinct messages (zkp_bls_verify_grouped_batch): signatures grp_off[g] .. grp_off[g + 1]
        sign msgs[g].  The answer of bls_verify on the messages expanded per signature with the same rand, from m hashes and m + 1 Miller
        loops.  Host arrays return a bool; resident torch tensors fill and return all_ok (int32 (1,)) without synchronising."""
        flags = _lib.BLS_POINTS_CHECKED if points_checked else 0
        if _is_torch(pk):
            import torch
            self._t_check(pk, 12, "pk"), self._t_check(sig, 24, "sig")
            n = pk.numel() // 12
            msgs, offsets, m, dst = self._msgs_t(msgs, offsets, dst)
            self._t_check(grp_off, None, "grp_off", rows=m + 1)
            if sig.numel() // 24 != n:
                raise ValueError("%d public keys, %d signatures" % (n, sig.numel() // 24))
            self._t_bytes(inf_pk, n, "inf_pk"), self._t_bytes(inf_sig, n, "inf_sig")
            if rand is None:
                rand = torch.from_numpy(self.rlc_random(n).view(np.int64)).to(pk.device)
            self._t_check(rand, 2, "rand", rows=n)
            if all_ok is None:
                all_ok = torch.empty(1, dtype=torch.int32, device=pk.device)
            self._t_check(all_ok, None, "all_ok", rows=1, dtypes=(torch.int32,))
            self._chk(self._lib.zkp_bls_verify_grouped_batch_dev(self._h, self._tp(pk), self._tp(inf_pk), self._tp(grp_off), self._tp(msgs), self._tp(offsets), m,
                                                                 self._tp(dst), dst.numel(), self._tp(sig), self._tp(inf_sig), n, self._tp(rand), flags,
                                                                 self._tp(all_ok), self._stream()))
            return all_ok
        buf, off, m, d = self._msgs_np(msgs, offsets, dst)
        pk, sig = _np(pk, 12), _np(sig, 24)
        n = pk.shape[0]
        grp_off = self._offsets_np(grp_off, "grp_off")
        if sig.shape[0] != n or grp_off.size != m + 1:
            raise ValueError("%d public keys, %d signatures, %d messages, %d group offsets" % (n, sig.shape[0], m, grp_off.size))
        ip, isg = _flags(inf_pk, n, "inf_pk"), _flags(inf_sig, n, "inf_sig")
        r = self.rlc_random(n) if rand is None else _np(rand, 2)
        if r.shape[0] != n:
            raise ValueError("rand holds %d pairs for %d signatures" % (r.shape[0], n))
        ok = ctypes.c_int(0)
        self._chk(self._lib.zkp_bls_verify_grouped_batch(self._h, _ptr(pk), _ptr(ip), _ptr(grp_off), _ptr(buf), _ptr(off), m, _ptr(d), d.size, _ptr(sig), _ptr(isg),
                                                         n, _ptr(r), flags, ctypes.byref(ok)))
        return bool(ok.value)

    def bls_fast_aggregate_verify_grouped(self, table, idx, seg_off, grp_off, msgs, sig, dst, offsets=None, inf_sig=None, rand=None, points_checked=False,
                                          all_ok=None):
        """n aggregate signatures ORDERED BY MESSAGE, each by the committee idx[seg_off[i] .. seg_off[i + 1]) of the key table, over m
        distinct messages (zkp_bls_fast_aggregate_verify_grouped_batch): the answer of bls_fast_aggregate_verify on the messages expanded
        per aggregate.  The arguments of bls_fast_aggregate_verify and bls_verify_grouped."""
        flags = _lib.BLS_POINTS_CHECKED if points_checked else 0
        if _is_torch(table):
            import torch
            n_table, n_idx, n = self._entries_t(table, idx, seg_off)
            self._t_check(sig, 24, "sig")
            msgs, offsets, m, dst = self._msgs_t(msgs, offsets, dst)
            self._t_check(grp_off, None, "grp_off", rows=m + 1)
            if sig.numel() // 24 != n:
                raise ValueError("%d committees, %d signatures" % (n, sig.numel() // 24))
            self._t_bytes(inf_sig, n, "inf_sig")
            if rand is None:
                rand = torch.from_numpy(self.rlc_random(n).view(np.int64)).to(table.device)
            self._t_check(rand, 2, "rand", rows=n)
            if all_ok is None:
                all_ok = torch.empty(1, dtype=torch.int32, device=table.device)
            self._t_check(all_ok, None, "all_ok", rows=1, dtypes=(torch.int32,))
            self._chk(self._lib.zkp_bls_fast_aggregate_verify_grouped_batch_dev(self._h, self._tp(table), n_table, self._tp(idx), n_idx, self._tp(seg_off),
                                                                                self._tp(grp_off), self._tp(msgs), self._tp(offsets), m, self._tp(dst),
                                                                                dst.numel(), self._tp(sig), self._tp(inf_sig), n, self._tp(rand), flags,
                                                                                self._tp(all_ok), self._stream()))
            return all_ok
        table, sig = _np(table, 12), _np(sig, 24)
        idx, seg_off = self._entries_np(idx, seg_off)
        buf, off, m, d = self._msgs_np(msgs, offsets, dst)
        n = seg_off.size - 1
        grp_off = self._offsets_np(grp_off, "grp_off")
        if sig.shape[0] != n or grp_off.size != m + 1:
            raise ValueError("%d committees, %d signatures, %d messages, %d group offsets" % (n, sig.shape[0], m, grp_off.size))
        isg = _flags(inf_sig, n, "inf_sig")
        r = self.rlc_random(n) if rand is None else _np(rand, 2)
        if r.shape[0] != n:
            raise ValueError("rand holds %d pairs for %d signatures" % (r.shape[0], n))
        ok = ctypes.c_int(0)
        self._chk(self._lib.zkp_bls_fast_aggregate_verify_grouped_batch(self._h, _ptr(table), table.shape[0], _ptr(idx), idx.size, _ptr(seg_off), _ptr(grp_off),
                                                                        _ptr(buf), _ptr(off), m, _ptr(d), d.size, _ptr(sig), _ptr(isg), n, _ptr(r), flags,
                                                                        ctypes.byref(ok)))
        return bool(ok.value)

    # ------------------------------------------------------------------ the Groth16 producer side (include/zkp_prove.h)
    def _csr(self, mat, name, keep, resident):
        """(n_rows, n_cols, row_ptr, col, val) -> zkp_fr_csr; row_ptr (n_rows + 1) and col (nnz) 32-bit, val (nnz, 4) canonical"""
        n_rows, n_cols, row_ptr, col, val = mat
        n_rows, n_cols = int(n_rows), int(n_cols)
        if n_rows < 0 or n_cols < 0:
            raise ValueError("%s: negative shape" % name)
        rec = _lib.FrCsr(n_rows=n_rows, n_cols=n_cols)
        if resident:
            import torch
            i32 = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)
            self._t_check(col, None, name + ".col", dtypes=i32)
            nnz = col.numel()
            self._t_check(val, 4, name + ".val", rows=nnz)
            self._t_check(row_ptr, None, name + ".row_ptr", rows=n_rows + 1, dtypes=i32)
            if val.numel() != nnz * 4 or row_ptr.numel() != n_rows + 1:
                raise ValueError("%s: %d row bounds, %d columns, %d values for %d rows" % (name, row_ptr.numel(), nnz, val.numel() // 4, n_rows))
            rec.nnz, rec.row_ptr, rec.col, rec.val = nnz, row_ptr.data_ptr(), col.data_ptr() if nnz else None, val.data_ptr() if nnz else None
            return rec
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint32).reshape(-1)
        col = np.ascontiguousarray(col, dtype=np.uint32).reshape(-1)
        val = _np(val, 4)
        if row_ptr.size != n_rows + 1 or val.shape[0] != col.size:
            raise ValueError("%s: %d row bounds, %d columns, %d values for %d rows" % (name, row_ptr.size, col.size, val.shape[0], n_rows))
        keep += [row_ptr, col, val]
        rec.nnz, rec.row_ptr, rec.col, rec.val = col.size, row_ptr.ctypes.data, col.ctypes.data if col.size else None, val.ctypes.data if col.size else None
        return rec

    def _r1cs(self, log2_n, n_inputs, a, b, c, keep, resident):
        rec = _lib.R1cs(log2_n=int(log2_n), n_inputs=int(n_inputs))
        rec.a, rec.b, rec.c = (self._csr(x, name, keep, resident) for x, name in ((a, "a"), (b, "b"), (c, "c")))
        if not 0 <= int(log2_n) <= 63 or int(n_inputs) < 0:
            raise ValueError("log2_n or n_inputs out of range")
        return rec

    def fr_spmv(self, mat, x, out_stride=None):
        """out (n, out_stride, 4): the sparse matrix mat = (n_rows, n_cols, row_ptr, col, val) in compressed rows times n dense vectors x
        (n, n_cols, 4) over Fr (zkp_fr_spmv_batch): out[j][k] = sum_e val[e] x[j][col[e]] over row k, zero from n_rows to out_stride
        (default n_rows).  Canonical in, canonical out.  Host arrays have their matrix checked (ZkpError on a malformed one); resident
        torch tensors (all of them) stay on the GPU, where a malformed matrix reads nothing outside its arrays and sets the
        validation word."""
        n_rows, n_cols = int(mat[0]), int(mat[1])
        out_stride = n_rows if out_stride is None else int(out_stride)
        resident = _is_torch(x)
        keep = []
        rec = self._csr(mat, "mat", keep, resident)
        if out_stride < 0:
            raise ValueError("out_stride is negative")
        if resident:
            import torch
            self._t_check(x, 4, "x")
            if n_cols == 0 or x.numel() % (4 * n_cols):
                raise ValueError("x holds no whole number of vectors of %d elements" % n_cols)
            n = x.numel() // (4 * n_cols)
            out = torch.empty((n, out_stride, 4), dtype=x.dtype, device=x.device)
            self._chk(self._lib.zkp_fr_spmv_batch_dev(self._h, ctypes.byref(rec), self._tp(x), n, out_stride, self._tp(out), self._stream()))
            return out
        x = np.ascontiguousarray(x, dtype=np.uint64)
        if n_cols == 0 or x.size % (4 * n_cols):
            raise ValueError("x holds no whole number of vectors of %d elements" % n_cols)
        n = x.size // (4 * n_cols)
        out = np.empty((n, out_stride, 4), dtype=np.uint64)
        self._chk(self._lib.zkp_fr_spmv_batch(self._h, ctypes.byref(rec), _ptr(x), n, out_stride, _ptr(out)))
        return out

    def groth16_quotient(self, log2_n, n_inputs, a, b, c, witness):
        """(h (n, N, 4), sat (n,) uint8): the QAP quotient of n witnesses (n, m, 4) of the constraint system A, B, C (each a matrix
        tuple as in fr_spmv, n_rows x m) over the N = 2^log2_n-point domain (zkp_groth16_quotient_batch): h = (a b - c) / (X^N - 1)
        by its N coefficients, natural order, and sat[j] = 1 iff witness j satisfies every row.  Resident torch tensors stay on the
        GPU."""
        resident = _is_torch(witness)
        keep = []
        rec = self._r1cs(log2_n, n_inputs, a, b, c, keep, resident)
        m, big_n = int(a[1]), 1 << int(log2_n)
        if resident:
            import torch
            self._t_check(witness, 4, "witness")
            if m == 0 or witness.numel() % (4 * m):
                raise ValueError("the witnesses hold no whole number of vectors of %d elements" % m)
            n = witness.numel() // (4 * m)
            h = torch.empty((n, big_n, 4), dtype=witness.dtype, device=witness.device)
            sat = torch.empty(n, dtype=torch.uint8, device=witness.device)
            self._chk(self._lib.zkp_groth16_quotient_batch_dev(self._h, ctypes.byref(rec), self._tp(witness), n, self._tp(h), self._tp(sat), self._stream()))
            return h, sat
        w = np.ascontiguousarray(witness, dtype=np.uint64)
        if m == 0 or w.size % (4 * m):
            raise ValueError("the witnesses hold no whole number of vectors of %d elements" % m)
        n = w.size // (4 * m)
        h, sat = np.empty((n, big_n, 4), dtype=np.uint64), np.empty(n, dtype=np.uint8)
        self._chk(self._lib.zkp_groth16_quotient_batch(self._h, ctypes.byref(rec), _ptr(w), n, _ptr(h), _ptr(sat)))
        return h, sat

    _PK_FIELDS = (("alpha_g1", 12), ("beta_g1", 12), ("delta_g1", 12), ("beta_g2", 24), ("delta_g2", 24), ("a_query", 12), ("a_inf", None), ("b_g1_query", 12),
                  ("b_g1_inf", None), ("b_g2_query", 24), ("b_g2_inf", None), ("l_query", 12), ("l_inf", None), ("h_query", 12))

    def groth16_prove(self, log2_n, n_inputs, a, b, c, pk, witness, rs):
        """n Groth16 proofs of one circuit (zkp_groth16_prove_batch): the constraint system as in groth16_quotient, the proving key pk a
        mapping of zkp_groth16_pk's field names to wire arrays (alpha_g1 / beta_g1 / delta_g1 (12,), beta_g2 / delta_g2 (24,), a_query
        and b_g1_query (m, 12), b_g2_query (m, 24), l_query (m - n_inputs - 1, 12), h_query (N - 1, 12), optional infinity bytes
        a_inf / b_g1_inf / b_g2_inf / l_inf), witnesses (n, m, 4) and the blinding scalars rs (n, 2, 4) - draw them uniformly and fresh
        per proof.  -> (A (n, 12), inf_a, B (n, 24), inf_b, C (n, 12), inf_c, sat): what groth16_verify_batch consumes, and sat[j] = 1 iff
        witness j satisfies the system.  The key points are trusted.  Resident torch tensors (all of them) stay on the GPU."""
        resident = _is_torch(witness)
        keep = []
        rec = self._r1cs(log2_n, n_inputs, a, b, c, keep, resident)
        m, big_n, l = int(a[1]), 1 << int(log2_n), int(n_inputs)
        rows = {"a_query": m, "a_inf": m, "b_g1_query": m, "b_g1_inf": m, "b_g2_query": m, "b_g2_inf": m, "l_query": m - l - 1, "l_inf": m - l - 1,
                "h_query": big_n - 1}
        if m - l - 1 < 0:
            raise ValueError("n_inputs + 1 exceeds the number of variables")
        key = _lib.Groth16Pk()
        for name, w in self._PK_FIELDS:
            x = pk.get(name)
            cnt = rows.get(name, 1)
            if x is None or cnt == 0:
                if w is not None and cnt:
                    raise ValueError("the proving key lacks %s" % name)
                continue
            if resident:
                if w is None:
                    self._t_bytes(x, cnt, name)
                else:
                    self._t_check(x, w, name, rows=cnt)
                setattr(key, name, x.data_ptr())
            else:
                arr = _flags(x, cnt, name) if w is None else _np(x, w)
                if w is not None and arr.shape[0] != cnt:
                    raise ValueError("%s holds %d points, %d expected" % (name, arr.shape[0], cnt))
                keep.append(arr)
                setattr(key, name, arr.ctypes.data)
        if resident:
            import torch
            self._t_check(witness, 4, "witness")
            if m == 0 or witness.numel() % (4 * m):
                raise ValueError("the witnesses hold no whole number of vectors of %d elements" % m)
            n = witness.numel() // (4 * m)
            self._t_check(rs, 8, "rs", rows=n)
            dev, dt = witness.device, witness.dtype
            pa, pb, pc = (torch.empty((n, w), dtype=dt, device=dev) for w in (12, 24, 12))
            ia, ib, ic, sat = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(4))
            self._chk(self._lib.zkp_groth16_prove_batch_dev(self._h, ctypes.byref(rec), ctypes.byref(key), self._tp(witness), self._tp(rs), n, 0, self._tp(pa),
                                                            self._tp(ia), self._tp(pb), self._tp(ib), self._tp(pc), self._tp(ic), self._tp(sat), self._stream()))
            return pa, ia, pb, ib, pc, ic, sat
        w = np.ascontiguousarray(witness, dtype=np.uint64)
        if m == 0 or w.size % (4 * m):
            raise ValueError("the witnesses hold no whole number of vectors of %d elements" % m)
        n = w.size // (4 * m)
        rs = _np(rs, 8)
        if rs.shape[0] != n:
            raise ValueError("rs holds %d pairs for %d witnesses" % (rs.shape[0], n))
        pa, pb, pc = (np.empty((n, cols), dtype=np.uint64) for cols in (12, 24, 12))
        ia, ib, ic, sat = (np.empty(n, dtype=np.uint8) for _ in range(4))
        self._chk(self._lib.zkp_groth16_prove_batch(self._h, ctypes.byref(rec), ctypes.byref(key), _ptr(w), _ptr(rs), n, 0, _ptr(pa), _ptr(ia), _ptr(pb), _ptr(ib),
                                                    _ptr(pc), _ptr(ic), _ptr(sat)))
        return pa, ia, pb, ib, pc, ic, sat

    def kzg_verify_batch(self, g1, g2, tau_g2, c, z, y, proof, *, inf_c=None, inf_proof=None, rand=None, points_checked=False, vk_checked=False):
        """n KZG openings against one setup as ONE check (zkp_kzg_verify_batch): setup points g1 (12,), g2 / tau_g2 (24,); commitments c
        and proofs (n, 12); points z and values y (n, 4).  True iff the random combination holds, every point is valid (unless
        points_checked / vk_checked), every z and y is below r and no (a_i, b_i) is zero; a batch with a false opening passes with
        probability <= 2^-128.  rand (n, 2) uint64, by default fresh from os.urandom (rlc_random) - never a seeded generator.  Host
        arrays return a bool; resident torch tensors (all of them) an int32 tensor (1,) without synchronising."""
        n = (c.numel() if _is_torch(c) else np.asarray(c).size) // 12
        if n == 0:
            return True
        if rand is None:
            rand = self.rlc_random(n)
        flags = (_lib.KZG_POINTS_CHECKED if points_checked else 0) | (_lib.KZG_VK_CHECKED if vk_checked else 0)
        vk_arrays = [("g1", g1, 12, 1), ("g2", g2, 24, 1), ("tau_g2", tau_g2, 24, 1)]
        b_arrays = [("c", c, 12, n), ("inf_c", inf_c, None, n), ("proof", proof, 12, n), ("inf_proof", inf_proof, None, n), ("z", z, 4, n), ("y", y, 4, n)]
        vk = _lib.KzgVk()
        bt = _lib.KzgBatch(n=n)
        if _is_torch(c):
            import torch
            dev = torch.device("cuda", self.device)
            for rec, arrays in ((vk, vk_arrays), (bt, b_arrays)):
                for name, x, w, rows in arrays:
                    if x is None:
                        continue
                    if w is None:
                        self._t_bytes(x, rows, name)
                    else:
                        self._t_check(x, w, name, rows=rows)
                        if x.numel() != rows * w:
                            raise ValueError("%s holds %d elements, %d expected" % (name, x.numel() // w, rows))
                    setattr(rec, name, x.data_ptr())
            if not _is_torch(rand):
                rand = torch.from_numpy(np.ascontiguousarray(rand, dtype=np.uint64).reshape(-1).view(np.int64)).to(dev)
            self._t_check(rand, 2, "rand", rows=n)
            all_ok = torch.empty(1, dtype=torch.int32, device=dev)
            self._chk(self._lib.zkp_kzg_verify_batch_dev(self._h, ctypes.byref(vk), ctypes.byref(bt), self._tp(rand), flags, self._tp(all_ok), self._stream()))
            return all_ok
        keep = []
        for rec, arrays in ((vk, vk_arrays), (bt, b_arrays)):
            for name, x, w, rows in arrays:
                if x is None:
                    continue
                arr = _flags(x, rows, name) if w is None else _np(x, w)
                if w is not None and arr.shape[0] != rows:
                    raise ValueError("%s holds %d elements, %d expected" % (name, arr.shape[0], rows))
                keep.append(arr)
                setattr(rec, name, arr.ctypes.data)
        r = _np(rand, 2)
        if r.shape[0] != n:
            raise ValueError("rand holds %d pairs for %d openings" % (r.shape[0], n))
        res = ctypes.c_int(0)
        self._chk(self._lib.zkp_kzg_verify_batch(self._h, ctypes.byref(vk), ctypes.byref(bt), _ptr(r), flags, ctypes.byref(res)))
        return bool(res.value)

    def msm_profile(self, which, points, scalars, n_msm=1, shared_bases=False):
        """measurement: one MSM on torch tensors with the milliseconds of its six phases (zkp_msm_profile_dev)"""
        import torch
        cols = 12 if which == 1 else 24
        self._t_check(scalars, 4, "scalars"), self._t_check(points, cols, "points")
        m = self._msm_shape(points.numel() // cols, scalars.numel() // 4, n_msm, shared_bases)
        out = torch.empty((n_msm, cols), dtype=scalars.dtype, device=scalars.device)
        oi = torch.empty(n_msm, dtype=torch.uint8, device=scalars.device)
        ms = (ctypes.c_float * 6)()
        self._chk(self._lib.zkp_msm_profile_dev(self._h, int(which), self._tp(points), None, self._tp(scalars), m, int(n_msm), 1 if shared_bases else 0,
                                                self._tp(out), self._tp(oi), self._stream(), ms))
        return out, oi, list(ms)

    def decode_points(self, data, which):
        """uncompressed big-endian bytes -> (points, inf, status); which = 1 (G1, 96 B) or 2 (G2, 192 B)"""
        size = 96 if which == 1 else 192
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        if buf.size % size:
            raise ValueError("byte string is not a multiple of %d bytes" % size)
        n = buf.size // size
        pts = np.empty((n, size // 8), dtype=np.uint64)
        inf, st = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8)
        fn = self._lib.zkp_g1_decode_batch if which == 1 else self._lib.zkp_g2_decode_batch
        self._chk(fn(self._h, _ptr(buf), n, _ptr(pts), _ptr(inf), _ptr(st)))
        return pts, inf, st

    def encode_points(self, pts, which, inf=None):
        cols = 12 if which == 1 else 24
        pts = _np(pts, cols)
        n = pts.shape[0]
        i = _flags(inf, n, "inf")
        out = np.empty(n * cols * 8, dtype=np.uint8)
        fn = self._lib.zkp_g1_encode_batch if which == 1 else self._lib.zkp_g2_encode_batch
        self._chk(fn(self._h, _ptr(pts), _ptr(i), n, _ptr(out)))
        return out.tobytes()

    # ---- BASELINE config 5 in one call, and the codec on resident tensors
    POINT_STATUS = ("ok", "non_canonical", "malformed", "not_on_curve", "not_in_subgroup")

    def points_check(self, g1_bytes, g2_bytes, k, st1=None, st2=None, ok=None, all_ok=None):
        """raw uncompressed points -> decode -> is_valid -> pairing check (zkp_points_check_batch[_dev]).
        numpy uint8 arrays (n x 96, n x 192): returns (st1, st2, ok, all_ok bool).  torch uint8 tensors on the engine's GPU:
        fills the given st1 / st2 / ok (uint8) and all_ok (int32[1]) tensors - each optional - asynchronously, returns None."""
        return self._points_check(g1_bytes, g2_bytes, k, st1, st2, ok, all_ok, compressed=False)

    def points_check_compressed(self, g1_bytes, g2_bytes, k, st1=None, st2=None, ok=None, all_ok=None):
        """points_check on compressed points (n x 48, n x 96 bytes; zkp_points_check_compressed_batch[_dev]): decompression is the
        decode step, status 3 (no square root) is "not on curve"; the same return values / tensor conventions as points_check"""
        return self._points_check(g1_bytes, g2_bytes, k, st1, st2, ok, all_ok, compressed=True)

    def _points_check(self, g1_bytes, g2_bytes, k, st1, st2, ok, all_ok, compressed):
        sz1 = 48 if compressed else 96
        sz2 = 2 * sz1
        if _is_torch(g1_bytes):
            import torch
            u8 = (torch.uint8,)
            self._t_check(g1_bytes, sz1, "g1_bytes", dtypes=u8), self._t_check(g2_bytes, sz2, "g2_bytes", dtypes=u8)
            n = g1_bytes.numel() // sz1
            if g2_bytes.numel() // sz2 != n or k <= 0 or n % k:
                raise ValueError("byte strings / k do not match")
            self._t_bytes(st1, n, "st1"), self._t_bytes(st2, n, "st2"), self._t_bytes(ok, n // k, "ok")
            if all_ok is not None:
                self._t_check(all_ok, None, "all_ok", rows=1, dtypes=(torch.int32,))
            fn = self._lib.zkp_points_check_compressed_batch_dev if compressed else self._lib.zkp_points_check_batch_dev
            self._chk(fn(self._h, self._tp(g1_bytes), self._tp(g2_bytes), n // k, k, self._tp(st1), self._tp(st2), self._tp(ok), self._tp(all_ok),
                         self._stream()))
            return None
        b1 = np.ascontiguousarray(g1_bytes, dtype=np.uint8).reshape(-1, sz1)
        b2 = np.ascontiguousarray(g2_bytes, dtype=np.uint8).reshape(-1, sz2)
        n = b1.shape[0]
        if b2.shape[0] != n or k <= 0 or n % k:
            raise ValueError("byte strings / k do not match")
        s1, s2, okb = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8), np.empty(n // k, dtype=np.uint8)
        allok = ctypes.c_int(1)
        fn = self._lib.zkp_points_check_compressed_batch if compressed else self._lib.zkp_points_check_batch
        self._chk(fn(self._h, _ptr(b1), _ptr(b2), n // k, k, _ptr(s1), _ptr(s2), _ptr(okb), ctypes.byref(allok)))
        return s1, s2, okb, bool(allok.value)

    def decode_points_dev(self, data, which):
        """uint8 tensor of uncompressed points on the engine's GPU -> (points int64 (n, 12 | 24), inf uint8, status uint8) tensors"""
        import torch
        size = 96 if which == 1 else 192
        self._t_check(data, size, "bytes", dtypes=(torch.uint8,))
        n = data.numel() // size
        pts = torch.empty((n, size // 8), dtype=torch.int64, device=data.device)
        inf = torch.empty(n, dtype=torch.uint8, device=data.device)
        st = torch.empty(n, dtype=torch.uint8, device=data.device)
        fn = self._lib.zkp_g1_decode_batch_dev if which == 1 else self._lib.zkp_g2_decode_batch_dev
        self._chk(fn(self._h, self._tp(data), n, self._tp(pts), self._tp(inf), self._tp(st), self._stream()))
        return pts, inf, st

    def encode_points_dev(self, pts, which, inf=None):
        """(n, 12 | 24) point tensor on the engine's GPU -> (n, 96 | 192) uint8 tensor of uncompressed big-endian points"""
        import torch
        cols = 12 if which == 1 else 24
        self._t_check(pts, cols, "points")
        n = pts.numel() // cols
        self._t_bytes(inf, n, "inf")
        out = torch.empty((n, cols * 8), dtype=torch.uint8, device=pts.device)
        fn = self._lib.zkp_g1_encode_batch_dev if which == 1 else self._lib.zkp_g2_encode_batch_dev
        self._chk(fn(self._h, self._tp(pts), self._tp(inf), n, self._tp(out), self._stream()))
        return out

    # ---- compressed points (48 B per G1 point, 96 B per G2 point) and the square roots behind them
    def fp_sqrt(self, a):
        """Fp::sqrt (reference src/fp.rs:280-300) of (n, 6) canonical elements -> (roots (n, 6), is_square (n,) uint8); the root is
        the reference's a^((p+1)/4), zero where the reference returns Err"""
        return self._sqrt(a, 1)

    def fp2_sqrt(self, a):
        """Fp2::sqrt (reference src/fp2.rs:231-273) of (n, 12) elements (c0 | c1) -> (roots (n, 12), is_square (n,) uint8), bit for bit
        the reference's root, zero where it returns None"""
        return self._sqrt(a, 2)

    def _sqrt(self, a, which):
        a = _np(a, 6 * which)
        out, sq = np.empty_like(a), np.empty(a.shape[0], dtype=np.uint8)
        fn = self._lib.zkp_fp_sqrt_batch if which == 1 else self._lib.zkp_fp2_sqrt_batch
        self._chk(fn(self._h, _ptr(a), a.shape[0], _ptr(out), _ptr(sq)))
        return out, sq

    def decompress_points(self, data, which):
        """compressed big-endian bytes -> (points, inf, status); which = 1 (G1, 48 B) or 2 (G2, 96 B).  status: 0 ok, 1 x >= p,
        2 malformed flags, 3 no square root (not on the curve); the subgroup is not checked"""
        size = 48 * which
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        if buf.size % size:
            raise ValueError("byte string is not a multiple of %d bytes" % size)
        n = buf.size // size
        pts = np.empty((n, 12 * which), dtype=np.uint64)
        inf, st = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8)
        fn = self._lib.zkp_g1_decompress_batch if which == 1 else self._lib.zkp_g2_decompress_batch
        self._chk(fn(self._h, _ptr(buf), n, _ptr(pts), _ptr(inf), _ptr(st)))
        return pts, inf, st

    def compress_points(self, pts, which, inf=None):
        """(n, 12 | 24) points -> compressed bytes (48 | 96 per point: x, the compression flag and the sort flag of y)"""
        cols = 12 * which
        pts = _np(pts, cols)
        n = pts.shape[0]
        i = _flags(inf, n, "inf")
        out = np.empty(n * 48 * which, dtype=np.uint8)
        fn = self._lib.zkp_g1_compress_batch if which == 1 else self._lib.zkp_g2_compress_batch
        self._chk(fn(self._h, _ptr(pts), _ptr(i), n, _ptr(out)))
        return out.tobytes()

    def decompress_points_dev(self, data, which):
        """uint8 tensor of compressed points on the engine's GPU -> (points int64 (n, 12 | 24), inf uint8, status uint8) tensors"""
        import torch
        size = 48 * which
        self._t_check(data, size, "bytes", dtypes=(torch.uint8,))
        n = data.numel() // size
        pts = torch.empty((n, 12 * which), dtype=torch.int64, device=data.device)
        inf = torch.empty(n, dtype=torch.uint8, device=data.device)
        st = torch.empty(n, dtype=torch.uint8, device=data.device)
        fn = self._lib.zkp_g1_decompress_batch_dev if which == 1 else self._lib.zkp_g2_decompress_batch_dev
        self._chk(fn(self._h, self._tp(data), n, self._tp(pts), self._tp(inf), self._tp(st), self._stream()))
        return pts, inf, st

    def compress_points_dev(self, pts, which, inf=None):
        """(n, 12 | 24) point tensor on the engine's GPU -> (n, 48 | 96) uint8 tensor of compressed points"""
        import torch
        cols = 12 * which
        self._t_check(pts, cols, "points")
        n = pts.numel() // cols
        self._t_bytes(inf, n, "inf")
        out = torch.empty((n, 48 * which), dtype=torch.uint8, device=pts.device)
        fn = self._lib.zkp_g1_compress_batch_dev if which == 1 else self._lib.zkp_g2_compress_batch_dev
        self._chk(fn(self._h, self._tp(pts), self._tp(inf), n, self._tp(out), self._stream()))
        return out

    # ---- one rank per GPU: the RCCL communicator behind the C ABI (the torch.distributed flavour is zkvm_pairings_amd/dist.py)
    @staticmethod
    def comm_unique_id():
        """128 bytes made on rank 0; every rank hands the same bytes to comm_init_rank"""
        buf = ctypes.create_string_buffer(128)
        st = _lib.load().zkp_comm_unique_id(buf)
        if st != 0:
            raise _lib.ZkpError(st, "zkp_comm_unique_id")
        return buf.raw

    def comm_init_rank(self, nranks, rank, unique_id):
        if len(unique_id) != 128:
            raise ValueError("the communicator id is 128 bytes")
        self._chk(self._lib.zkp_comm_init_rank(self._h, int(nranks), int(rank), ctypes.c_char_p(bytes(unique_id))))

    def comm_destroy(self):
        self._chk(self._lib.zkp_comm_destroy(self._h))

    def comm_info(self):
        n, r = ctypes.c_int(), ctypes.c_int()
        self._chk(self._lib.zkp_comm_info(self._h, ctypes.byref(n), ctypes.byref(r)))
        return n.value, r.value

    def _join_failed(self, entry, dev_flag=None):
        """a LOCAL argument error found on this side of the ABI (sizes that do not match, k that does not divide n) must not keep the
        rank out of the collective its peers are already waiting in: enter it through the same entry point with arguments the library
        itself refuses (no points, one check) - it then takes part with flag 0 / the zero record - and let the caller raise afterwards"""
        null = ctypes.c_void_p(None)
        out = ctypes.c_int(0)
        if entry == "check":
            rc = self._lib.zkp_pairing_check_batch_allreduce(self._h, null, null, null, null, 1, 1, null, ctypes.byref(out))
        elif entry == "check_dev":
            rc = self._lib.zkp_pairing_check_batch_allreduce_dev(self._h, null, null, null, null, 1, 1, null, self._tp(dev_flag), self._stream())
        elif entry == "gt_check_dev":
            rc = self._lib.zkp_pairing_gt_check_batch_allreduce_dev(self._h, null, null, null, null, 1, 1, null, null, self._tp(dev_flag), self._stream())
        elif entry == "points":
            rc = self._lib.zkp_points_check_batch_allreduce(self._h, null, null, 1, 1, null, null, null, ctypes.byref(out))
        else:
            rc = self._lib.zkp_pairing_product_check_allgather(self._h, null, null, null, null, 1, null, ctypes.byref(out))
        # the library refuses the arguments (ZKP_ERR_ARG = -1) AFTER it has taken part in the collective; ZKP_ERR_COMM (-6) means there
        # was no communicator / RCCL failed, i.e. nothing was joined - the caller's error should say so
        self.last_join_status = rc
        return rc

    def and_allreduce(self, flag):
        """in-place AND (all-reduce MIN) of an int32[1] tensor of {0,1} over the communicator's ranks, on the current stream"""
        import torch
        self._t_check(flag, None, "flag", rows=1, dtypes=(torch.int32,))
        self._chk(self._lib.zkp_and_allreduce_dev(self._h, self._tp(flag), self._stream()))

    def pairing_check_allreduce(self, g1, g2, k, inf1=None, inf2=None):
        """this rank's block of a sharded check + the AND over all ranks (zkp_pairing_check_batch_allreduce[_dev]):
        -> (ok bytes of this rank's checks, all_ok over ALL ranks: bool for host arrays, int32[1] tensor for device tensors)"""
        if _is_torch(g1):
            import torch
            allok = torch.empty(1, dtype=torch.int32, device=torch.device("cuda", self.device))
            try:
                n = self._t_pairs(g1, g2, inf1, inf2, k)
            except (TypeError, ValueError):
                self._join_failed("check_dev", allok)
                raise
            ok = torch.empty(n // k, dtype=torch.uint8, device=g1.device)
            self._chk(self._lib.zkp_pairing_check_batch_allreduce_dev(self._h, self._tp(g1), self._tp(g2), self._tp(inf1), self._tp(inf2), n // k, k,
                                                                      self._tp(ok), self._tp(allok), self._stream()))
            return ok, allok
        try:
            g1, g2 = _np(g1, 12), _np(g2, 24)
            n = g1.shape[0]
            if g2.shape[0] != n or k <= 0 or n % k:
                raise ValueError("g1 / g2 sizes do not match or are not a multiple of k")
            i1, i2 = _flags(inf1, n, "inf1"), _flags(inf2, n, "inf2")
        except (TypeError, ValueError):
            self._join_failed("check")
            raise
        ok = np.empty(n // k, dtype=np.uint8)
        allok = ctypes.c_int(1)
        self._chk(self._lib.zkp_pairing_check_batch_allreduce(self._h, _ptr(g1), _ptr(g2), _ptr(i1), _ptr(i2), n // k, k, _ptr(ok), ctypes.byref(allok)))
        return ok, bool(allok.value)

    def pairing_gt_check_allreduce(self, g1, g2, k, out_gt, ok, all_ok, inf1=None, inf2=None):
        """device tensors only: pairing_gt_check of this rank's block + the AND over all ranks in all_ok (int32[1], required) -
        zkp_pairing_gt_check_batch_allreduce_dev, BASELINE config 3 as one call per rank"""
        import torch
        try:
            self._t_check(all_ok, None, "all_ok", rows=1, dtypes=(torch.int32,))
        except (TypeError, ValueError, AttributeError):
            # a flag tensor this rank cannot even hand to the library (wrong dtype / shape / device, not a tensor): the peers are waiting
            # in the collective all the same - join it with a flag of the wrapper's own, then raise
            self._join_failed("gt_check_dev", torch.empty(1, dtype=torch.int32, device=torch.device("cuda", self.device)))
            raise
        try:
            n = self._t_pairs(g1, g2, inf1, inf2, k)
            if out_gt is not None:
                self._t_check(out_gt, 72, "out_gt", rows=n // k)
            self._t_bytes(ok, n // k, "ok")
        except (TypeError, ValueError):
            self._join_failed("gt_check_dev", all_ok)
            raise
        self._chk(self._lib.zkp_pairing_gt_check_batch_allreduce_dev(self._h, self._tp(g1), self._tp(g2), self._tp(inf1), self._tp(inf2), n // k, k,
                                                                     self._tp(out_gt), self._tp(ok), self._tp(all_ok), self._stream()))

    def points_check_allreduce(self, g1_bytes, g2_bytes, k):
        """config 5 on a node: this rank's block of points_check + the AND over all ranks (host arrays) -> (st1, st2, ok, all_ok)"""
        try:
            b1 = np.ascontiguousarray(g1_bytes, dtype=np.uint8).reshape(-1, 96)
            b2 = np.ascontiguousarray(g2_bytes, dtype=np.uint8).reshape(-1, 192)
            n = b1.shape[0]
            if b2.shape[0] != n or k <= 0 or n % k:
                raise ValueError("byte strings / k do not match")
        except (TypeError, ValueError):
            self._join_failed("points")
            raise
        s1, s2, okb = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8), np.empty(n // k, dtype=np.uint8)
        allok = ctypes.c_int(1)
        self._chk(self._lib.zkp_points_check_batch_allreduce(self._h, _ptr(b1), _ptr(b2), n // k, k, _ptr(s1), _ptr(s2), _ptr(okb), ctypes.byref(allok)))
        return s1, s2, okb, bool(allok.value)

    def pairing_product_check_allgather(self, g1, g2, inf1=None, inf2=None):
        try:
            g1, g2 = _np(g1, 12), _np(g2, 24)
            n = g1.shape[0]
            if g2.shape[0] != n:
                raise ValueError("g1 and g2 hold different numbers of points")
            i1, i2 = _flags(inf1, n, "inf1"), _flags(inf2, n, "inf2")
        except (TypeError, ValueError):
            self._join_failed("product")
            raise
        gt = np.empty(72, dtype=np.uint64)
        one = ctypes.c_int(0)
        self._chk(self._lib.zkp_pairing_product_check_allgather(self._h, _ptr(g1), _ptr(g2), _ptr(i1), _ptr(i2), n, _ptr(gt), ctypes.byref(one)))
        return gt, bool(one.value)

    FP_OPS = {"mul": 0, "add": 1, "sub": 2, "neg": 3, "square": 4, "invert": 5}
    TOWER_OPS = {"fp2_mul": 0, "fp2_square": 1, "fp6_mul": 2, "fp6_square": 3, "fp6_frobenius": 4, "fp12_mul": 5, "fp12_square": 6,
                 "fp12_mul_by_014": 7, "fp12_frobenius": 8, "fp12_conjugate": 9, "fp12_cyclotomic_square": 10, "fp12_cyclotomic_pow2k": 11, "fp12_cyclotomic_decompress": 12,
                 "fp2_invert": 13, "fp2_mul_by_nonresidue": 14, "fp2_mul_fp": 15, "fp6_mul_by_1": 16, "fp6_mul_by_01": 17, "fp6_mul_by_nonresidue": 18,
                 "fp6_invert": 19, "fp12_invert": 20}

    def fp_op(self, op, a, b=None, core28=False):
        """zkVM-precompile-shaped batched field op: op 0 = mul, 1 = add (reference src/fp.rs:376,443), 2 sub, 3 neg,
        4 square, 5 invert (or the names in FP_OPS); core28 runs it on the 28-bit core of the cooperative family."""
        op = self.FP_OPS.get(op, op)
        a = _np(a, 6)
        b = None if b is None else _np(b, 6)
        if b is not None and b.shape != a.shape:
            raise ValueError("fp_op: operand shapes differ")
        out = np.empty_like(a)
        self._chk(self._lib.zkp_fp_op_batch(self._h, int(op) | (16 if core28 else 0), _ptr(a), _ptr(b), a.shape[0], _ptr(out)))
        return out

    def tower_op(self, op, a, b=None, repeat=1):
        """one tower operation per (n,72) record on the engine's kernel family (zkp_tower_op_batch); op: name in TOWER_OPS"""
        op = self.TOWER_OPS.get(op, op)
        a = _np(a, 72)
        b = None if b is None else _np(b, 72)
        if b is not None and b.shape != a.shape:
            raise ValueError("tower_op: operand shapes differ")
        out = np.empty_like(a)
        self._chk(self._lib.zkp_tower_op_batch(self._h, int(op), _ptr(a), _ptr(b), a.shape[0], int(repeat), _ptr(out)))
        return out

    # ------------------------------------------------------------------ torch (device-resident) API
    def _t_check(self, t, cols, name="tensor", rows=None, dtypes=None):
        """every tensor handed to a *_dev entry point: on this engine's GPU, contiguous, 64-bit words (or bytes), and
        large enough - a wrong-sized or CPU tensor would otherwise become an out-of-bounds access in HBM"""
        import torch
        if not _is_torch(t):
            raise TypeError("%s: expected a torch tensor" % name)
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError("%s must live on cuda:%d" % (name, self.device))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
        if t.dtype not in (dtypes or (torch.int64, torch.uint64)):
            raise ValueError("%s has dtype %s" % (name, t.dtype))
        if cols is not None and t.numel() % cols:
            raise ValueError("%s: %d elements is not a multiple of %d" % (name, t.numel(), cols))
        if rows is not None and t.numel() < rows * (cols or 1):
            raise ValueError("%s: %d elements, %d needed" % (name, t.numel(), rows * (cols or 1)))
        return t

    def _t_bytes(self, t, n, name):
        import torch
        return None if t is None else self._t_check(t, None, name, rows=n, dtypes=(torch.uint8,))

    def _t_pairs(self, g1, g2, inf1, inf2, k=1):
        self._t_check(g1, 12, "g1"), self._t_check(g2, 24, "g2")
        n = g1.numel() // 12
        if g2.numel() // 24 != n:
            raise ValueError("g1 holds %d points, g2 %d" % (n, g2.numel() // 24))
        if k <= 0 or n % k:
            raise ValueError("%d pairs is not a positive multiple of k = %d" % (n, k))
        self._t_bytes(inf1, n, "inf1"), self._t_bytes(inf2, n, "inf2")
        return n

    @staticmethod
    def _tp(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    @staticmethod
    def _stream():
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _pairing_t(self, g1, g2, inf1, inf2, out=None):
        import torch
        n = self._t_pairs(g1, g2, inf1, inf2)
        if out is None:
            out = torch.empty((n, 72), dtype=g1.dtype, device=g1.device)
        self._t_check(out, 72, "out", rows=n)
        self._chk(self._lib.zkp_pairing_batch_dev(self._h, self._tp(g1), self._tp(g2), self._tp(inf1), self._tp(inf2), n, self._tp(out), self._stream()))
        return out

    def _miller_t(self, g1, g2, k, inf1, inf2):
        import torch
        n = self._t_pairs(g1, g2, inf1, inf2, k)
        out = torch.empty((n // k, 72), dtype=g1.dtype, device=g1.device)
        self._chk(self._lib.zkp_multi_miller_loop_batch_dev(self._h, self._tp(g1), self._tp(g2), self._tp(inf1), self._tp(inf2), n // k, k, self._tp(out), self._stream()))
        return out

    def _fexp_t(self, f):
        import torch
        self._t_check(f, 72, "f")
        out = torch.empty_like(f)
        self._chk(self._lib.zkp_final_exponentiation_batch_dev(self._h, self._tp(f), f.numel() // 72, self._tp(out), self._stream()))
        return out

    def _check_t(self, g1, g2, k, inf1, inf2):
        import torch
        n = self._t_pairs(g1, g2, inf1, inf2, k)
        ok = torch.empty(n // k, dtype=torch.uint8, device=g1.device)
        allok = torch.empty(1, dtype=torch.int32, device=g1.device)
        self._chk(self._lib.zkp_pairing_check_batch_dev(self._h, self._tp(g1), self._tp(g2), self._tp(inf1), self._tp(inf2), n // k, k, self._tp(ok), self._tp(allok), self._stream()))
        return ok, allok

    def pairing_gt_check(self, g1, g2, k, out_gt, ok, all_ok, inf1=None, inf2=None):
        """device tensors only: Gt out + ok bytes + AND flag in one fused pass (bench step); out_gt / ok / all_ok are each optional"""
        import torch
        n = self._t_pairs(g1, g2, inf1, inf2, k)
        if out_gt is not None:
            self._t_check(out_gt, 72, "out_gt", rows=n // k)
        self._t_bytes(ok, n // k, "ok")
        if all_ok is not None:
            self._t_check(all_ok, None, "all_ok", rows=1, dtypes=(torch.int32,))
        self._chk(self._lib.zkp_pairing_gt_check_batch_dev(self._h, self._tp(g1), self._tp(g2), self._tp(inf1), self._tp(inf2), n // k, k,
                                                           self._tp(out_gt), self._tp(ok), self._tp(all_ok), self._stream()))

    def _valid_t(self, pts, inf, which):
        import torch
        cols = 12 if which == 1 else 24
        self._t_check(pts, cols, "points")
        n = pts.numel() // cols
        self._t_bytes(inf, n, "inf")
        st = torch.empty(n, dtype=torch.uint8, device=pts.device)
        fn = self._lib.zkp_g1_is_valid_batch_dev if which == 1 else self._lib.zkp_g2_is_valid_batch_dev
        self._chk(fn(self._h, self._tp(pts), self._tp(inf), n, self._tp(st), self._stream()))
        return st

    def _mul_t(self, base, scalars, which):
        import torch
        cols = 12 if which == 1 else 24
        self._t_check(scalars, 4, "scalars")
        n = scalars.numel() // 4
        if not _is_torch(base):
            base = torch.from_numpy(np.ascontiguousarray(base, dtype=np.uint64).view(np.int64)).to(scalars.device)
        base = base.contiguous().view(-1)
        self._t_check(base, cols, "base")
        stride = 0 if base.numel() == cols and n != 1 else cols
        if stride and base.numel() != n * cols:
            raise ValueError("base holds %d points, %d scalars given" % (base.numel() // cols, n))
        out = torch.empty((n, cols), dtype=scalars.dtype, device=scalars.device)
        oi = torch.empty(n, dtype=torch.uint8, device=scalars.device)
        fn = self._lib.zkp_g1_mul_batch_dev if which == 1 else self._lib.zkp_g2_mul_batch_dev
        self._chk(fn(self._h, self._tp(base), stride, self._tp(scalars), n, self._tp(out), self._tp(oi), self._stream()))
        return out, oi

    def clock_probe(self, stream, spin_us=20000):
        """queue the one-wavefront clock probe on `stream` (a torch.cuda.Stream); -> (tensor of two int64: shader-clock
        ticks, wall-clock ticks; valid once the stream has drained, wall clock rate in kHz)"""
        import torch
        out = torch.empty(2, dtype=torch.int64, device=torch.device("cuda", self.device))   # no fill: nothing queued on another stream may touch it
        khz = ctypes.c_int(0)
        self._chk(self._lib.zkp_clock_probe_dev(self._h, ctypes.c_void_p(stream.cuda_stream), int(spin_us), self._tp(out), ctypes.byref(khz)))
        return out, khz.value

    def time_coop_step(self, which, n):
        """ms of one launch of a diagnostic / single-kernel timing run (zkp_time_coop_step)"""
        ms = ctypes.c_float()
        self._chk(self._lib.zkp_time_coop_step(self._h, int(which), int(n), ctypes.byref(ms)))
        return ms.value

    PROFILE_CLASSES = ("k_prep_lines", "k_coop<30,4> miller", "k_coop<24,34> fexp_a", "k_batch_inv", "k_ksq", "k_kdec_a", "k_kdec_b",
                       "k_coop<36,24> hard-part step programs", "k_coop<24,34> phase-C step programs")

    def profile_pairing(self, g1, g2, out):
        """one pass of the fused pairing with every launch timed on its own (zkp_profile_pairing_dev) -> {class: (ms, launches)}"""
        n = self._t_pairs(g1, g2, None, None)
        self._t_check(out, 72, "out", rows=n)
        k = len(self.PROFILE_CLASSES)
        ms, cnt = (ctypes.c_float * k)(), (ctypes.c_int * k)()
        self._chk(self._lib.zkp_profile_pairing_dev(self._h, self._tp(g1), self._tp(g2), n, self._tp(out), ms, cnt))
        return {name: (ms[i], cnt[i]) for i, name in enumerate(self.PROFILE_CLASSES)}

    def time_pairing(self, g1, g2, out, reps):
        """avg ms per launch of the fused pairing kernel, HIP events on the engine's own stream."""
        n = self._t_pairs(g1, g2, None, None)
        self._t_check(out, 72, "out", rows=n)
        ms = ctypes.c_float()
        self._chk(self._lib.zkp_time_pairing_dev(self._h, self._tp(g1), self._tp(g2), g1.numel() // 12, self._tp(out), int(reps), ctypes.byref(ms)))
        return ms.value
