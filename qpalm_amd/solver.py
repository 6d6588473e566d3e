"""Host-side mirror of the reference's Python interface on top of the gfx950 C ABI.

`Qpalm` mirrors interfaces/python/qpalm.py:192-375 (set_default_settings / set_data / _allocate_work ==
qpalm_setup / _solve / _warm_start / _update_bounds / _update_q) for ONE QP; `QpalmBatch` is the
batched form the MI355X engine is built for (B independent QPs of equal dimensions resident in HBM).
Neither class contains numerics: everything runs in the HIP kernels behind include/qpalm_gfx950.h.
"""
import collections
import ctypes as C
import time
import weakref

import numpy as np

from . import capi
from .capi import Info, QpgError, Settings, Stats, f64, fptr, i64, iptr

SOLVED, DUAL_TERMINATED, MAX_ITER_REACHED = 1, 2, -2
PRIMAL_INFEASIBLE, DUAL_INFEASIBLE, TIME_LIMIT_REACHED, UNSOLVED, ERROR = -3, -4, -5, -10, 0


class Context:
    def __init__(self, device=0, lib_path=None, **options):
        self.L = capi.load(lib_path)
        h = C.c_void_p()
        self._check(self.L.qpg_ctx_create(int(device), C.byref(h)))
        self.h = h
        self.device = int(device)
        for k, v in options.items():
            self.set_option(k, v)

    def _check(self, rc):
        if rc != 0:
            raise QpgError(rc, self.L.qpg_last_error().decode())

    def set_option(self, name, value):
        self._check(self.L.qpg_ctx_set_option(self.h, name.encode(), int(value)))

    @property
    def backend(self):
        return self.L.qpg_backend_name().decode()

    def default_settings(self, **kw):
        s = Settings()
        self.L.qpg_set_default_settings(C.byref(s))
        for k, v in kw.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s

    def hbm_copy_gbs(self, nbytes=1 << 30, reps=5):
        """measured copy bandwidth of the device (GB/s, read + write): the attainable-HBM yardstick of bench.py"""
        g = C.c_float(0.0)
        self._check(self.L.qpg_ctx_hbm_copy_gbs(self.h, int(nbytes), int(reps), C.byref(g)))
        return float(g.value)

    def pinned_array(self, shape):
        """float64 array of zeros in page-locked host memory (qpg_host_alloc): hand bounds over / take solutions in such
        arrays and the copies are DMA transfers.  The memory lives as long as the array (and this context)."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        count = int(np.prod(shape)) if shape else 1
        p = C.c_void_p()
        self._check(self.L.qpg_host_alloc(self.h, max(count, 1) * 8, C.byref(p)))
        buf = (C.c_double * max(count, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.float64, count=count).reshape(shape)
        ctx_l, ctx_h, addr = self.L, self.h, p.value
        weakref.finalize(buf, lambda: ctx_l.qpg_host_free(ctx_h, C.c_void_p(addr)))
        return arr

    def hbm_read_gbs(self, nbytes=1 << 30, reps=5):
        """measured read-only streaming bandwidth of the device (GB/s)"""
        g = C.c_float(0.0)
        self._check(self.L.qpg_ctx_hbm_read_gbs(self.h, int(nbytes), int(reps), C.byref(g)))
        return float(g.value)

    def close(self):
        if self.h:
            self.L.qpg_ctx_destroy(self.h)
            self.h = None


# The arrays of the per-step device calls, one row each, in the field order of the call's struct (capi.Device*; DeviceStep.warm and DevicePolish.store
# are values, not arrays).  key: an input's name in error messages, an output's key in `want` / `out`.  width: an attribute of the batch (n, m, nnzQ,
# nnzA), 1 (a scalar per member) or 4.  per_dir: the array gains the leading K of adjoints_device / tangents_device; `active` (in and out) does not.
_Row = collections.namedtuple("_Row", "field key width dtype out per_dir")


def _in(field, width, dtype="float64", per_dir=False, key=None):
    return _Row(field, key or field, width, dtype, False, per_dir)


def _out(key, width, dtype="float64", per_dir=False):
    return _Row("active_out" if key == "active" else key, key, width, dtype, True, per_dir)


_SENS_OUT = (_out("active", "m", "int64"), _out("flag", 1, "int64", True), _out("resid", 1, per_dir=True), _out("passes", 1, "int64", True))
_CALLS = dict(
    step=(capi.DeviceStep, (_in("bmin", "m"), _in("bmax", "m"), _in("q", "n"), _in("warm_x", "n", key="warm x"), _in("warm_y", "m", key="warm y"),
                            _out("x", "n"), _out("y", "m"), _out("status_val", 1, "int64"), _out("iter", 1, "int64"), _out("rejected", 1, "int64"))),
    adjoint=(capi.DeviceAdjoint, (_in("gx", "n", per_dir=True), _in("gy", "m", per_dir=True), _in("active_in", "m", "int64", key="active"),
                                  _out("dq", "n", per_dir=True), _out("dbmin", "m", per_dir=True), _out("dbmax", "m", per_dir=True),
                                  _out("dQx", "nnzQ", per_dir=True), _out("dAx", "nnzA", per_dir=True)) + _SENS_OUT),
    tangent=(capi.DeviceTangent, (_in("dq", "n", per_dir=True), _in("dbmin", "m", per_dir=True), _in("dbmax", "m", per_dir=True),
                                  _in("dQx", "nnzQ", per_dir=True), _in("dAx", "nnzA", per_dir=True), _in("active_in", "m", "int64", key="active"),
                                  _out("dx", "n", per_dir=True), _out("dy", "m", per_dir=True)) + _SENS_OUT),
    polish=(capi.DevicePolish, (_in("active_in", "m", "int64"), _out("x", "n"), _out("y", "m"), _out("res", 4)) + _SENS_OUT))
for _struct, _arrays in _CALLS.values():   # the rows are the struct's arrays, in its order: _io fills the struct by position
    assert [r.field for r in _arrays] == [f for f, kind in _struct._fields_ if kind is C.c_void_p], _struct


class QpalmBatch:
    """B QPs  min 1/2 x'Qx + q'x + c  s.t. bmin <= Ax <= bmax  with common (n, m)."""

    def __init__(self, ctx, problems, settings=None):
        """problems: sequence of objects with .args() -> (n, m, Qp, Qi, Qx, Ap, Ai, Ax, q, bmin, bmax) and .c"""
        self.ctx, self.L = ctx, ctx.L
        self.B = len(problems)
        self.n, self.m = max(int(p.n) for p in problems), max(int(p.m) for p in problems)
        self.dims = [(int(p.n), int(p.m)) for p in problems]   # members may be smaller than the batch (mixed sizes)
        nnzA = max(int(p.Ap[-1]) for p in problems)
        nnzQ = max(int(p.Qp[-1]) for p in problems)
        self.nnzA, self.nnzQ = nnzA, nnzQ   # row lengths of the arrays update_Q_A takes
        self.settings = settings if settings is not None else ctx.default_settings()
        self.epoch = 0   # counts the calls that change what adjoint_device differentiates (solves, warm starts, updates): torch_layer checks it
        # counts the calls that change the values of Q and A (a setup, update_Q_A*): a point recorded under another count is no longer valid for
        # adjoint_device / tangent_device(at=...)
        self.matrix_epoch = 1
        self._row_cache = {}   # _rows
        self._emulated = ctx.backend == "host-emulation"   # device memory is host memory there; asked once: the per-step calls check every array
        h = C.c_void_p()
        t0 = time.perf_counter()
        self._check(self.L.qpg_batch_create(ctx.h, self.B, self.n, self.m, nnzA, nnzQ, C.byref(self.settings), C.byref(h)))
        self.h = h
        # every member in ONE call (qpg_batch_set_problems: arrays of pointers, the conversion to the device layout runs on host threads)
        B = self.B
        keep = []   # contiguous int64 / float64 views stay alive until the call returns
        cols = [(C.c_void_p * B)() for _ in range(9)]
        for b, p in enumerate(problems):
            arrs = (i64(p.Qp), i64(p.Qi), f64(p.Qx), i64(p.Ap), i64(p.Ai), f64(p.Ax), f64(p.q), f64(p.bmin), f64(p.bmax))
            keep.append(arrs)
            for k, a in enumerate(arrs):
                cols[k][b] = a.ctypes.data
        ns, ms = i64([int(p.n) for p in problems]), i64([int(p.m) for p in problems])
        cs = f64([float(getattr(p, "c", 0.0)) for p in problems])
        self._check(self.L.qpg_batch_set_problems(self.h, 0, B, iptr(ns), iptr(ms), cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], cols[6],
                                                   fptr(cs), cols[7], cols[8]))
        del keep
        t1 = time.perf_counter()
        self._check(self.L.qpg_batch_setup(self.h))
        # what qpalm_setup does (src/qpalm.c:73-319), split as this engine does it: host-side copies / format conversion of every
        # member (qpg_batch_set_problem), then packing + upload + the device part (Ruiz scaling, derived copies; qpg_batch_setup)
        self.set_problem_s, self.batch_setup_s = t1 - t0, time.perf_counter() - t1

    def _check(self, rc):
        if rc != 0:
            raise QpgError(rc, self.L.qpg_last_error().decode())

    # -- qpalm.h API ---------------------------------------------------------------------------
    def warm_start(self, x=None, y=None):
        self.epoch += 1
        xs = f64(x).reshape(self.B, self.n) if x is not None else None
        ys = f64(y).reshape(self.B, self.m) if y is not None else None
        self._check(self.L.qpg_batch_warm_start(self.h, fptr(xs) if xs is not None else None, fptr(ys) if ys is not None else None))

    def warm_start_last(self):
        """qpalm_warm_start of every QP with its own last solution, device-resident (the MPC receding-horizon step)."""
        self.epoch += 1
        self._check(self.L.qpg_batch_warm_start_last(self.h))

    def solve(self):
        self.epoch += 1
        self._check(self.L.qpg_batch_solve(self.h))

    def iterate(self, k=1):
        self.epoch += 1
        self._check(self.L.qpg_batch_iterate(self.h, int(k)))

    def last_solve_ms(self):
        ms = C.c_float(0.0)
        self._check(self.L.qpg_batch_last_solve_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def launch_shape(self):
        """(concurrent workgroups, threads per workgroup, LDS bytes per workgroup) of this batch."""
        w, t, l = capi.c_int(0), capi.c_int(0), capi.c_int(0)
        self._check(self.L.qpg_batch_launch_shape(self.h, C.byref(w), C.byref(t), C.byref(l)))
        return int(w.value), int(t.value), int(l.value)

    def sparse_info(self, b=0):
        """(nnz(L) of member b's sparse factor, bytes of the device block of all sparse factors); raises on a batch with dense factors"""
        z, d = capi.c_int(0), capi.c_int(0)
        self._check(self.L.qpg_batch_sparse_info(self.h, int(b), C.byref(z), C.byref(d)))
        return int(z.value), int(d.value)

    def sparse_perm(self, b=0):
        """(perm, levels): the ordering of member b's sparse factor (perm[new] = old; identity = natural) and the height of its elimination tree.
        The factor has n rows, n + m in KKT mode (factorization_method = 0: P K P' with K in the [x; y] numbering)"""
        n, m = self.dims[b]
        perm = np.zeros(n + m if int(self.settings.factorization_method) == 0 else n, dtype=np.int64)
        lev = capi.c_int(0)
        self._check(self.L.qpg_batch_sparse_perm(self.h, int(b), perm.ctypes.data_as(C.POINTER(capi.c_int)), C.byref(lev)))
        return perm, int(lev.value)

    def sparse_factor(self, b=0):
        """(Lp, Li, Lx, D) of member b's sparse factor as it stands on the device, in the factor's own numbering (sparse_perm maps it): column
        pointers (nf + 1; nf = n, or n + m in KKT mode), row indices and values of the strict lower part, pivots.  Raises on a batch with dense
        factors (factor() reads those) and when the batch has more members than factor slots"""
        n, m = self.dims[b]
        nf = n + m if int(self.settings.factorization_method) == 0 else n
        nnz = self.sparse_info(b)[0]
        Lp, Li = np.zeros(nf + 1, dtype=np.int64), np.zeros(nnz, dtype=np.int64)
        Lx, D = np.zeros(nnz), np.zeros(nf)
        self._check(self.L.qpg_batch_get_sparse_factor(self.h, int(b), iptr(Lp), iptr(Li), fptr(Lx), fptr(D)))
        return Lp, Li, Lx, D

    def sparse_coop_info(self, b=0):
        """(factor_launches, solve_launches, max_grid): member b's launch plan under the context option "sparse_coop" = 1; (0, 0, 0) when the batch runs
        on one workgroup per QP; raises on a batch with dense factors"""
        f, s, g = capi.c_int(0), capi.c_int(0), capi.c_int(0)
        self._check(self.L.qpg_batch_sparse_coop_info(self.h, int(b), C.byref(f), C.byref(s), C.byref(g)))
        return int(f.value), int(s.value), int(g.value)

    def num_unfinished(self):
        c = capi.c_int(0)
        self._check(self.L.qpg_batch_num_unfinished(self.h, C.byref(c)))
        return int(c.value)

    def update_settings(self, s):
        self.epoch += 1
        rc = self.L.qpg_batch_update_settings(self.h, C.byref(s))
        if rc == 0:
            self.settings = s
        return rc

    def update_bounds(self, bmin=None, bmax=None):
        self.epoch += 1
        a = f64(bmin).reshape(self.B, self.m) if bmin is not None else None
        b = f64(bmax).reshape(self.B, self.m) if bmax is not None else None
        return self.L.qpg_batch_update_bounds(self.h, fptr(a) if a is not None else None, fptr(b) if b is not None else None)

    def update_q(self, q):
        self.epoch += 1
        q = f64(q).reshape(self.B, self.n)
        self._check(self.L.qpg_batch_update_q(self.h, fptr(q)))

    def _padded(self, v, width):
        """[B][width] float64 from an array of that shape or a list of per-member arrays (padded with zeros)"""
        if isinstance(v, np.ndarray) and v.ndim == 2:
            out = f64(v)
            if out.shape != (self.B, width):
                raise ValueError("expected an array of shape %r, got %r" % ((self.B, width), out.shape))
            return out
        if len(v) != self.B:
            raise ValueError("expected %d per-member arrays, got %d" % (self.B, len(v)))
        out = np.zeros((self.B, width))
        for b, row in enumerate(v):
            row = f64(row).ravel()
            if len(row) > width:
                raise ValueError("member %d: %d values, the batch holds at most %d" % (b, len(row), width))
            out[b, :len(row)] = row
        return out

    def update_Q_A(self, Qx, Ax):
        """qpalm_update_Q_A: new values of Q and A on the patterns the batch was set up with, each member's in the order of the Qx / Ax its problem was
        given with.  [B][nnzQ_max] / [B][nnzA_max] arrays, or lists of per-member arrays.  The batch is then what a fresh setup with these values, the
        latest q / bounds and the current settings would be; the stored solutions stay (warm_start_last)."""
        self.epoch += 1
        self.matrix_epoch += 1
        q, a = self._padded(Qx, self.nnzQ), self._padded(Ax, self.nnzA)
        self._check(self.L.qpg_batch_update_Q_A(self.h, fptr(q), fptr(a)))

    def update_Q_A_device(self, ptr_Qx, ptr_Ax):
        """the same from device memory: raw addresses of [B][nnzQ_max] / [B][nnzA_max] float64 arrays (e.g. torch tensors' data_ptr())"""
        self.epoch += 1
        self.matrix_epoch += 1
        self._check(self.L.qpg_batch_update_Q_A_device(self.h, C.c_void_p(int(ptr_Qx)), C.c_void_p(int(ptr_Ax))))

    # -- the per-step calls on arrays in device memory ---------------------------------------------------
    def _dev(self, v, shape, what, dtype="float64"):
        """(address or None, is_tensor) of an array in the context's device memory: None, a raw address (int, as update_Q_A_device takes) or a torch
        tensor, which must sit on the context's device, be contiguous and have this dtype and shape -- ValueError otherwise, before anything is
        launched.  Under emulation device memory is host memory: CPU tensors there."""
        if v is None:
            return None, False
        if isinstance(v, (int, np.integer)):
            return int(v), False
        if not hasattr(v, "data_ptr"):
            raise ValueError("%s: expected a torch tensor or a raw address, got %s" % (what, type(v).__name__))
        import torch
        want = getattr(torch, dtype)
        on_gpu = not self._emulated
        if v.device.type != ("cuda" if on_gpu else "cpu") or (on_gpu and v.device.index != self.ctx.device):
            raise ValueError("%s: tensor on %s, the batch lives on %s" % (what, v.device, "cuda:%d" % self.ctx.device if on_gpu else "cpu (emulation)"))
        if v.dtype != want:
            raise ValueError("%s: dtype %s, expected %s" % (what, v.dtype, want))
        if tuple(v.shape) != tuple(shape):
            raise ValueError("%s: shape %r, expected %r" % (what, tuple(v.shape), tuple(shape)))
        if not v.is_contiguous():
            raise ValueError("%s: tensor is not contiguous" % what)
        return int(v.data_ptr()), True

    def _dev_args(self, *specs):
        """addresses (c_void_p or None) of several arrays, all checked first; then, if any was a tensor, torch's current stream on the device is
        synchronised -- the calls are synchronous: whatever produced the inputs must have finished"""
        got = [self._dev(v, shape, what, dtype) for v, shape, what, dtype in specs]
        if any(t for _, t in got) and not self._emulated:
            import torch
            torch.cuda.current_stream(self.ctx.device).synchronize()
        return [C.c_void_p(a) if a is not None else None for a, _ in got]

    def _empty(self, shape, dtype="float64"):
        import torch
        dev = "cpu" if self._emulated else "cuda:%d" % self.ctx.device
        return torch.empty(shape, dtype=getattr(torch, dtype), device=dev)

    def update_bounds_device(self, bmin=None, bmax=None):
        """update_bounds from [B][m] float64 arrays in device memory (torch tensors or raw addresses); returns the code like update_bounds"""
        self.epoch += 1
        a, b = self._dev_args((bmin, (self.B, self.m), "bmin", "float64"), (bmax, (self.B, self.m), "bmax", "float64"))
        return self.L.qpg_batch_update_bounds_device(self.h, a, b)

    def update_q_device(self, q):
        self.epoch += 1
        if q is None:
            raise ValueError("q: expected a torch tensor or a raw address")
        a, = self._dev_args((q, (self.B, self.n), "q", "float64"))
        self._check(self.L.qpg_batch_update_q_device(self.h, a))

    def warm_start_device(self, x=None, y=None):
        self.epoch += 1
        a, b = self._dev_args((x, (self.B, self.n), "x", "float64"), (y, (self.B, self.m), "y", "float64"))
        self._check(self.L.qpg_batch_warm_start_device(self.h, a, b))

    def solution_device(self, out=None):
        """(x [B][n], y [B][m]) written in device memory; out = (x, y): tensors or raw addresses to fill (either may be None), else new tensors"""
        x, y = out if out is not None else (self._empty((self.B, self.n)), self._empty((self.B, self.m)))
        a, b = self._dev_args((x, (self.B, self.n), "x", "float64"), (y, (self.B, self.m), "y", "float64"))
        self._check(self.L.qpg_batch_get_solution_device(self.h, a, b))
        return x, y

    def status_device(self, out=None):
        """(status_val [B], iter [B]) as int64, written in device memory; out as for solution_device"""
        sv, it = out if out is not None else (self._empty((self.B,), "int64"), self._empty((self.B,), "int64"))
        a, b = self._dev_args((sv, (self.B,), "status_val", "int64"), (it, (self.B,), "iter", "int64"))
        self._check(self.L.qpg_batch_get_status_device(self.h, a, b))
        return sv, it

    STEP_OUT, ADJOINT_OUT, TANGENT_OUT, POLISH_OUT = (tuple(r.key for r in _CALLS[c][1] if r.out) for c in ("step", "adjoint", "tangent", "polish"))

    def _rows(self, call, K=None):
        """(inputs, outputs, value fields) of a device call of _CALLS in this batch: [(shape, name, dtype)] of its input arrays in struct order, as
        _dev_args takes them, {key: (shape, name, dtype)} of its outputs likewise, and the positions in the struct of the fields that are not arrays.
        The per-direction arrays have the leading K of a plural call.  Worked out once per (call, K): the calls are made every step."""
        got = self._row_cache.get((call, K))
        if got is None:
            def spec(r):
                shape = (self.B,) if r.width == 1 else (self.B, r.width if isinstance(r.width, int) else getattr(self, r.width))
                return ((K,) + shape if K is not None and r.per_dir else shape), ("out " + r.key if r.out else r.key), r.dtype
            struct, rows = _CALLS[call]
            values = [i for i, (_, kind) in enumerate(struct._fields_) if kind is not C.c_void_p]
            got = self._row_cache[call, K] = [spec(r) for r in rows if not r.out], {r.key: spec(r) for r in rows if r.out}, values
        return got

    def _outputs(self, call, want, out, K, err):
        """(out, specs) of a device call: the dict of its outputs -- `out` itself, or new tensors for the keys in `want` -- and the _dev_args specs of
        all its outputs in struct order (a key that is absent or None: not wanted).  A key the call does not have: ValueError(err ...)"""
        rows = self._rows(call, K)[1]
        unknown = set(out if out is not None else want) - set(rows) - {"n_selected"}
        if unknown:
            raise ValueError("%s %r" % (err, sorted(unknown)))
        if out is None:
            out = {k: self._empty(rows[k][0], rows[k][2]) for k in want}
        return out, [(out.get(k),) + spec for k, spec in rows.items()]

    def _zeros(self, call, keys, K=None):
        """zero-filled tensors for these outputs of a device call: an `out` whose rows stay zero where the call writes nothing"""
        rows = self._rows(call, K)[1]
        return {k: self._empty(rows[k][0], rows[k][2]).zero_() for k in keys}

    def _io(self, call, ins, specs, K=None, value=None):
        """the struct of a device call: its input arrays `ins` in struct order and its outputs' `specs`, all checked by _dev_args; `value`: its field
        that is not an array"""
        rows, _, values = self._rows(call, K)
        fields = self._dev_args(*[(v,) + spec for v, spec in zip(ins, rows)], *specs)
        for i in values:
            fields.insert(i, value)
        return _CALLS[call][0](*fields)

    def _check_select(self, select):
        if select is not None and (isinstance(select, (int, np.integer)) or not hasattr(select, "data_ptr")):
            raise ValueError("select: expected an int64 torch tensor of shape (%d,)" % self.B)

    def _route(self, name, io, select=None, at=None, K=None):
        """The entry point of a form of a device call; returns (rc, n_selected).  Nothing given: qpg_batch_<name>_device.  select ([B] int64 tensor on the
        batch's device, entries 0 / 1, validated like every other array): qpg_batch_<name>_subset_device.  at = (x, y, active), a recorded point:
        qpg_batch_<name>_at_device, which takes select itself.  K (the plural methods; None otherwise): qpg_batch_<name>_multi_device, select and at
        both optional."""
        fn = "qpg_batch_%s_" % name
        if select is None and at is None and K is None:
            return getattr(self.L, fn + "device")(self.h, C.byref(io)), self.B
        if at is not None and (not isinstance(at, (tuple, list)) or len(at) != 3 or any(v is None for v in at)):
            raise ValueError("at: expected (x, y, active), all three given")
        self._check_select(select)
        x, y, act = at if at is not None else (None, None, None)
        x, y, act, sel = self._dev_args((x, (self.B, self.n), "at x", "float64"), (y, (self.B, self.m), "at y", "float64"),
                                        (act, (self.B, self.m), "at active", "int64"), (select, (self.B,), "select", "int64"))
        point = C.byref(capi.DevicePoint(x, y, act)) if at is not None else None
        cnt = capi.c_int(0)
        if K is not None:
            rc = getattr(self.L, fn + "multi_device")(self.h, C.byref(io), K, point, sel, C.byref(cnt))
        elif at is not None:
            rc = getattr(self.L, fn + "at_device")(self.h, C.byref(io), point, sel, C.byref(cnt))
        else:
            rc = getattr(self.L, fn + "subset_device")(self.h, C.byref(io), sel, C.byref(cnt))
        return rc, int(cnt.value)

    def active_device(self, out=None, select=None):
        """The active set of the stored solutions ([B][m] int64 in device memory: -1 lower, +1 upper, 0 inactive; all zeros for a member that is not
        SOLVED / DUAL_TERMINATED) by the rule adjoint_device applies with active=None (qpg_batch_get_active_device): what its `active` output would
        hold, without the solve.  out: a tensor or raw address to fill, else a new tensor.  select: as for step_device -- only the rows of members with
        1 are written.  With x, y of solution_device it is the point `at=` of adjoint_device / tangent_device takes.  `epoch` stays."""
        if out is None:
            out = self._empty((self.B, self.m), "int64")
            if select is not None:
                out.zero_()
        a, = self._dev_args((out, (self.B, self.m), "out", "int64"))
        if select is None:
            self._check(self.L.qpg_batch_get_active_device(self.h, a))
        else:
            self._check_select(select)
            sel, = self._dev_args((select, (self.B,), "select", "int64"))
            self._check(self.L.qpg_batch_get_active_subset_device(self.h, a, sel, None))
        return out

    def step_device(self, bmin=None, bmax=None, q=None, warm="last", out=None, select=None):
        """One receding-horizon step without the host (qpg_batch_step_device): new bounds / q (None = unchanged), warm start ("last" = every QP's own
        last solution, None = none, (x, y) = given arrays, one of which may be None), solve, and the results written in device memory.  All arrays are
        torch tensors on the context's device or raw addresses.  out: a dict with any of the keys x, y, status_val, iter, rejected (absent or None =
        not wanted); without it all five are allocated.  Returns (rc, out): rc = 0, or -2 (QPG_ERR_INVALID) when some member's bounds were refused --
        the step has run all the same, that member on its old bounds, and out["rejected"] says which.
        select: None, or a [B] int64 tensor of 0 / 1 on the batch's device: only the members with 1 take the step (qpg_batch_step_subset_device,
        DESIGN.md section 15); the others are untouched -- their state, and their rows of every `out` array, which keep what they held (arrays
        allocated here hold uninitialised memory there).  With select the returned dict also holds n_selected (an int: how many members took the
        step; the key is ignored when the dict is handed in again); an entry other than 0 / 1, or a solve in progress, raises QpgError (-2)."""
        self.epoch += 1
        out, specs = self._outputs("step", self.STEP_OUT, out, None, "out: unknown keys")
        if warm is None:
            mode, wx, wy = 0, None, None
        elif isinstance(warm, str):
            if warm != "last":
                raise ValueError("warm: 'last', None or (x, y)")
            mode, wx, wy = 1, None, None
        else:
            mode = 2
            wx, wy = warm
            if wx is None and wy is None:
                raise ValueError("warm: (x, y) with both None")
        rc, cnt = self._route("step", self._io("step", (bmin, bmax, q, wx, wy), specs, value=mode), select)
        if rc not in (0, -2) or (rc == -2 and select is not None and b"Lower bound" not in self.L.qpg_last_error()):
            self._check(rc)
        if select is not None:
            out["n_selected"] = cnt
        return rc, out

    def _sens(self, name, dirs, active, want, out, select, at, plural=False, K=None):
        """the body of adjoint_device / adjoints_device (name "adjoint", dirs = (gx, gy)) and of tangent_device / tangents_device (name "tangent",
        dirs = (dq, dbmin, dbmax, dQx, dAx))"""
        method = name + ("s_device" if plural else "_device")
        if name == "adjoint":
            missing = "gx: expected a torch tensor or a raw address" if dirs[0] is None else None
        else:
            missing = "%s: no direction (dq, dbmin, dbmax, dQx and dAx are all None)" % method if all(v is None for v in dirs) else None
        if plural:   # K comes first: the outputs' shapes need it
            if missing:
                raise ValueError(missing)
            K = self._leading(method, K, *dirs)
        out, specs = self._outputs(name, want, out, K, method + ": unknown outputs")
        if missing:
            raise ValueError(missing)
        rc, cnt = self._route(name, self._io(name, dirs + (active,), specs, K), select, at, K)
        self._check(rc)
        if select is not None:
            out["n_selected"] = cnt
        return out

    def adjoint_device(self, gx, gy=None, active=None, want=ADJOINT_OUT, out=None, select=None, at=None):
        """Gradients of a loss through the stored solutions (qpg_batch_adjoint_device): gx = dl/dx [B][n], gy = dl/dy [B][m] or None, active = the active
        set to differentiate at ([B][m] int64: -1 lower, +1 upper, 0 inactive) or None for the engine's own test on the stored solution.  All arrays
        are torch tensors on the context's device or raw addresses.  want: which outputs to compute, among dq [B][n], dbmin / dbmax [B][m],
        dQx [B][nnzQ_max], dAx [B][nnzA_max] (the layout update_Q_A takes), active [B][m] int64 (the set used), flag [B] int64 (0 done, 1 pass cap /
        non-finite, 2 member not solved), resid [B], passes [B] int64.  out: a dict of tensors / addresses to fill instead (then `want` is ignored).
        Returns the dict.  select: as for step_device -- only the members with 1 are differentiated (qpg_batch_adjoint_subset_device); the rows of the
        others in every output, flag included, keep what they held, and the dict gains n_selected.
        at: None, or (x, y, active) -- a point recorded after an earlier solve of this batch (solution_device and active_device, or the `active` output
        of a sensitivity call made then): the gradients are those of THAT solve (qpg_batch_adjoint_at_device), however often the
        batch has been stepped since.  Valid while `matrix_epoch` is what it was at that solve; q, bounds, penalties and warm starts may differ.  The
        members' current statuses are not consulted (no flag 2): exclude members with select.  `active` must be None then."""
        return self._sens("adjoint", (gx, gy), active, want, out, select, at)

    def tangent_device(self, dq=None, dbmin=None, dbmax=None, dQx=None, dAx=None, active=None, want=TANGENT_OUT, out=None, select=None, at=None):
        """How the stored solutions move along one direction of the data (qpg_batch_tangent_device): dq [B][n], dbmin / dbmax [B][m], dQx [B][nnzQ_max],
        dAx [B][nnzA_max] (the layout update_Q_A takes); None = zero, at least one must be given.  active: as for adjoint_device.  All arrays are torch
        tensors on the context's device or raw addresses.  want: which outputs to compute, among dx [B][n], dy [B][m], active [B][m] int64 (the set
        used), flag [B] int64 (0 done, 1 pass cap / non-finite, 2 member not solved), resid [B], passes [B] int64.  out: a dict of tensors / addresses
        to fill instead (then `want` is ignored).  Returns the dict.  The batch's state (and `epoch`) stays: x + dx, y + dy is a first-order
        prediction of the next solution and can go straight into warm_start_device.  select: as for adjoint_device
        (qpg_batch_tangent_subset_device).  at: as for adjoint_device (qpg_batch_tangent_at_device)."""
        return self._sens("tangent", (dq, dbmin, dbmax, dQx, dAx), active, want, out, select, at)

    # -- K directions per call ---------------------------------------------------
    def _leading(self, what, K, *arrays):
        """K of a multi call: the leading dimension of the first tensor among `arrays`, which the others must share (their full shapes are checked
        by _dev_args); `K` itself when it is given, which raw addresses need"""
        for v in arrays:
            if hasattr(v, "data_ptr"):
                if v.dim() < 1:
                    raise ValueError("%s: expected a leading dimension K on every per-direction tensor" % what)
                k = int(v.shape[0])
                if K is not None and int(K) != k:
                    raise ValueError("%s: K = %d, but a tensor has the leading dimension %d" % (what, int(K), k))
                K = k
                break
        if K is None:
            raise ValueError("%s: K cannot be taken from raw addresses, pass K" % what)
        return int(K)

    def adjoints_device(self, gx, gy=None, active=None, want=ADJOINT_OUT, out=None, select=None, at=None, K=None):
        """adjoint_device for K pairs (gx, gy) in one call (qpg_batch_adjoint_multi_device): gx [K][B][n], gy [K][B][m] or None;
        the outputs dq, dbmin, dbmax, dQx, dAx, flag, resid and passes have the same leading K, `active` (input and output, [B][m]), select and at are
        those of adjoint_device and shared by the directions.  K is the leading dimension of gx (pass K when gx is a raw address).  Slice k of every
        output holds the bits adjoint_device returns for slice k of the inputs; the set-up, the factor and the host's checks are paid once.  A
        direction that fails is flagged in its own slice; a member that is not solved is flagged in all of them.  `epoch` stays."""
        return self._sens("adjoint", (gx, gy), active, want, out, select, at, True, K)

    def tangents_device(self, dq=None, dbmin=None, dbmax=None, dQx=None, dAx=None, active=None, want=TANGENT_OUT, out=None, select=None, at=None,
                        K=None):
        """tangent_device for K directions in one call (qpg_batch_tangent_multi_device): dq [K][B][n], dbmin / dbmax [K][B][m],
        dQx [K][B][nnzQ_max], dAx [K][B][nnzA_max]; None = zero in every direction, at least one must be given.  The outputs dx, dy, flag, resid and
        passes have the same leading K; `active` (input and output, [B][m]), select and at are those of tangent_device and shared by the directions.
        K is the leading dimension of the first tensor given (pass K with raw addresses).  Slice k of every output holds the bits tangent_device
        returns for slice k of the inputs.  `epoch` stays."""
        return self._sens("tangent", (dq, dbmin, dbmax, dQx, dAx), active, want, out, select, at, True, K)

    def jacobian_device(self, wrt="q", mode="tangent", chunk=16, active=None, select=None, at=None):
        """The Jacobian of the stored solutions with respect to q, bmin or bmax, column block by column block through the multi calls: a dict with
        dx [B][n][p], dy [B][m][p] (mode "tangent" only) and flag [B] (the largest flag over the directions), p = n for wrt "q" and m for "bmin" /
        "bmax".  mode "tangent": the directions are the unit vectors of the chosen input, at most `chunk` per call (p / chunk calls, the last one
        shorter).  mode "adjoint": the seeds are the unit vectors of x (gx = e_j, gy = None), and row j of dx is the dq / dbmin / dbmax of seed j --
        n solves instead of p.  A unit vector beyond a sized member's own n / m gives a zero column (row): the engine ignores such entries.  active,
        select and at: as for tangent_device; the rows of members that are not selected are zeros.  `epoch` stays."""
        import torch
        if wrt not in ("q", "bmin", "bmax"):
            raise ValueError("jacobian_device: wrt is 'q', 'bmin' or 'bmax'")
        if mode not in ("tangent", "adjoint"):
            raise ValueError("jacobian_device: mode is 'tangent' or 'adjoint'")
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError("jacobian_device: chunk must be at least 1")
        nB, n, m = self.B, self.n, self.m
        p = n if wrt == "q" else m
        res = dict(dx=self._empty((nB, n, p)).zero_(), flag=self._empty((nB,), "int64").zero_())
        if mode == "tangent":
            res["dy"] = self._empty((nB, m, p)).zero_()
        ndirs = p if mode == "tangent" else n   # tangent: unit vectors of the input; adjoint: unit vectors of x
        name = "d" + wrt
        for j0 in range(0, ndirs, chunk):
            kc = min(chunk, ndirs - j0)
            seed = self._empty((kc, nB, ndirs)).zero_()
            for k in range(kc):
                seed[k, :, j0 + k] = 1.0
            if mode == "tangent":
                out = self._zeros("tangent", ("dx", "dy", "flag"), kc)
                self.tangents_device(**{name: seed}, active=active, out=out, select=select, at=at)
                res["dx"][:, :, j0:j0 + kc] = out["dx"].permute(1, 2, 0)
                res["dy"][:, :, j0:j0 + kc] = out["dy"].permute(1, 2, 0)
            else:
                out = self._zeros("adjoint", (name, "flag"), kc)
                self.adjoints_device(seed, active=active, out=out, select=select, at=at)
                res["dx"][:, j0:j0 + kc, :] = out[name].permute(1, 0, 2)
            res["flag"] = torch.maximum(res["flag"], out["flag"].max(dim=0).values)
        return res

    @property
    def sens_penalty(self):
        """The penalty floor of adjoint_device, tangent_device and polish_device (qpg_batch_set_sens_penalty): the preconditioner of
        their refinement uses max(sigma_i, floor) on the active rows, which takes the pass cap away after a loose solve.  0 (the default): the solve's
        own penalties.  A setting of the linear solve alone: the batch's state and `epoch` stay."""
        v = C.c_double(0.0)
        self._check(self.L.qpg_batch_get_sens_penalty(self.h, C.byref(v)))
        return float(v.value)

    @sens_penalty.setter
    def sens_penalty(self, floor):
        self._check(self.L.qpg_batch_set_sens_penalty(self.h, float(floor)))

    def polish_device(self, active_in=None, store=False, want=POLISH_OUT, out=None, select=None):
        """The exact solution at the final active set (qpg_batch_polish_device): per member one correction solve from its stored solution, a clip of
        wrong-signed multipliers and a verdict.  active_in: as `active` of adjoint_device.  want: which outputs to compute, among x [B][n], y [B][m]
        (the candidate where accepted, the stored solution otherwise), res [B][4] (pri_old, dua_old, pri_new, dua_new), active [B][m] int64 (the set
        used), flag [B] int64 (0 accepted, 1 pass cap / non-finite, 2 member not solved, 3 candidate rejected), resid [B], passes [B] int64.  out: a
        dict of tensors / addresses to fill instead (then `want` is ignored).  store: accepted candidates become the members' stored solutions (what
        solution*, adjoint_device, tangent_device and warm_start_last read); info() still describes the solve.  Returns the dict.  `epoch` advances
        only when store changed a member (the flags then come to the host: one small transfer).  select: as for adjoint_device
        (qpg_batch_polish_subset_device): only selected members are polished and, with store, replaced; only their flags count for `epoch`."""
        out, specs = self._outputs("polish", want, out, None, "polish_device: unknown outputs")
        flag = out.get("flag")
        if store and not hasattr(flag, "data_ptr"):   # the flags decide whether the stored solutions moved
            flag = self._empty((self.B,), "int64")
            specs = self._outputs("polish", (), dict(out, flag=flag), None, "polish_device: unknown outputs")[1]
        rc, cnt = self._route("polish", self._io("polish", (active_in,), specs, value=1 if store else 0), select)
        self._check(rc)
        if store and bool(((flag == 0) if select is None else (flag == 0) & (select != 0)).any()):
            self.epoch += 1
        if select is not None:
            out["n_selected"] = cnt
        return out

    # -- results --------------------------------------------------------------------------------
    def info(self, b=0):
        out = Info()
        self._check(self.L.qpg_batch_get_info(self.h, int(b), C.byref(out)))
        return out

    def stats(self, b=0):
        out = Stats()
        self._check(self.L.qpg_batch_get_stats(self.h, int(b), C.byref(out)))
        return out

    def solution(self, out=None):
        """(x [B][n], y [B][m]); out = (x, y): C-contiguous float64 arrays to fill (e.g. Context.pinned_array: no page
        faults, DMA at PCIe rate) instead of fresh ones"""
        if out is None:
            x, y = np.zeros((self.B, self.n)), np.zeros((self.B, self.m))
        else:
            x, y = out
            assert x.shape == (self.B, self.n) and y.shape == (self.B, self.m) and x.dtype == np.float64 and y.dtype == np.float64
            assert x.flags.c_contiguous and y.flags.c_contiguous
        self._check(self.L.qpg_batch_get_solution(self.h, fptr(x), fptr(y)))
        return x, y

    def infos(self):
        """QPALMInfo of every QP (one device-to-host copy)."""
        out = (Info * self.B)()
        self._check(self.L.qpg_batch_get_info_all(self.h, out))
        return out

    def stats_all(self):
        out = (Stats * self.B)()
        self._check(self.L.qpg_batch_get_stats_all(self.h, out))
        return out

    def begin_solve(self):
        self.epoch += 1
        self._check(self.L.qpg_batch_begin_solve(self.h))

    def solution_of(self, k):
        """(x, y) of member k without the padding of a mixed-size batch"""
        x, y = self.solution()
        n, m = self.dims[k]
        return x[k, :n], y[k, :m]

    def statuses(self):
        return np.array([int(i.status_val) for i in self.infos()])

    _LEN_N = {"x", "Qx", "Aty", "x_prev", "x0", "Atyh", "df", "dphi", "dphi_prev", "d", "Qd", "delta_x", "temp_n", "D", "Dinv",
              "solution_x", "q"}

    def _veclen(self, name):
        if name in self._LEN_N:
            return self.n
        if name in ("delta", "alpha"):
            return 2 * self.m
        return self.m

    def vec(self, name, b=0):
        out = np.zeros(self._veclen(name))
        self._check(self.L.qpg_batch_get_vector(self.h, name.encode(), int(b), fptr(out), len(out)))
        return out

    def named_vec(self, name, length, b=0):
        """first `length` entries of a per-QP fp64 device array by its arena name (e.g. "At_sqrt_sigma")"""
        out = np.zeros(int(length))
        self._check(self.L.qpg_batch_get_vector(self.h, name.encode(), int(b), fptr(out), len(out)))
        return out

    def set_vec(self, name, v, b=0):
        v = f64(v)
        self._check(self.L.qpg_batch_set_vector(self.h, name.encode(), int(b), fptr(v), len(v)))

    def ivec(self, name, b=0, length=None):
        out = np.zeros(self.m if length is None else int(length), np.int64)
        if len(out):
            self._check(self.L.qpg_batch_get_ivector(self.h, name.encode(), int(b), iptr(out), len(out)))
        return out

    def set_ivec(self, name, v, b=0):
        v = i64(v)
        if len(v):
            self._check(self.L.qpg_batch_set_ivector(self.h, name.encode(), int(b), iptr(v), len(v)))

    def set_scalar(self, name, v, b=0):
        self._check(self.L.qpg_batch_set_scalar(self.h, name.encode(), int(b), float(v)))

    def factor(self, b=0):
        Lm, D = np.zeros((self.n, self.n)), np.zeros(self.n)
        self._check(self.L.qpg_batch_get_factor(self.h, int(b), fptr(Lm), fptr(D), self.n))
        return Lm.T.copy(), D  # column-major buffer -> [i, j]

    def factor_rows(self, rows, b=0):
        """(L, D) of a factor slot with `rows` rows: rows = n (Schur) or n + m (KKT mode)"""
        Lm, D = np.zeros((rows, rows)), np.zeros(rows)
        self._check(self.L.qpg_batch_get_factor(self.h, int(b), fptr(Lm), fptr(D), int(rows)))
        return Lm.T.copy(), D

    # -- solver_interface.h surface ---------------------------------------------------------------
    def mat_vec(self, which, x, b=0):
        x = f64(x)
        y = np.zeros(self.m if which == "A" else self.n)
        self._check(self.L.qpg_mat_vec(self.h, int(b), ord(which), fptr(x), fptr(y)))
        return y

    def mat_tpose_vec(self, which, x, b=0):
        x = f64(x)
        y = np.zeros(self.n)
        self._check(self.L.qpg_mat_tpose_vec(self.h, int(b), ord(which), fptr(x), fptr(y)))
        return y

    def op(self, name, b=0):
        self._check(getattr(self.L, "qpg_" + name)(self.h, int(b)))

    def coop_op_chains(self):
        """how many single operations of this batch (op: ldlchol, ldlcholQAtsigmaA, the three updates, ldlsolveLD_neg_dphi) have run on the coop
        grid kernels since it was created; 0 on a batch that is not in coop mode"""
        c = capi.c_int(0)
        self._check(self.L.qpg_batch_coop_op_chains(self.h, C.byref(c)))
        return int(c.value)

    def exact_linesearch(self, b=0):
        t = capi.c_float(0.0)
        self._check(self.L.qpg_exact_linesearch(self.h, int(b), C.byref(t)))
        return float(t.value)

    def ldlsolve_all(self, reps=1):
        ms = C.c_float(0.0)
        self._check(self.L.qpg_batch_ldlsolve_all(self.h, int(reps), C.byref(ms)))
        return float(ms.value)

    def sweep_probe(self, reps=1, nranks=16):
        """diagnostic: the update sweep alone on every resident workgroup (qpg_batch_sweep_probe); ms of the launch"""
        ms = C.c_float(0.0)
        self._check(self.L.qpg_batch_sweep_probe(self.h, int(reps), int(nranks), C.byref(ms)))
        return float(ms.value)

    def device_ptr(self, name):
        p, nbytes = C.c_void_p(), C.c_size_t(0)
        self._check(self.L.qpg_batch_device_ptr(self.h, name.encode(), C.byref(p), C.byref(nbytes)))
        return p.value, nbytes.value

    def close(self):
        if getattr(self, "h", None):
            self.L.qpg_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Qpalm:
    """Single-QP facade with the reference's Python class shape (interfaces/python/qpalm.py:192-375)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.settings = ctx.default_settings()
        self._prob = None
        self._batch = None

    def set_default_settings(self):
        self.settings = self.ctx.default_settings()

    def set_data(self, Q, A, q, bmin, bmax, c=0.0):
        """Q, A: scipy sparse (any format); only tril(Q) is read, like stype = -1."""
        import scipy.sparse as sp
        from .problems import QP
        Qc = sp.csc_matrix(sp.tril(sp.csc_matrix(Q)))
        Ac = sp.csc_matrix(A)
        Qc.sort_indices()
        Ac.sort_indices()
        self._prob = QP(Ac.shape[1], Ac.shape[0], Qc.indptr.astype(np.int64), Qc.indices.astype(np.int64),
                        Qc.data.astype(float), Ac.indptr.astype(np.int64), Ac.indices.astype(np.int64),
                        Ac.data.astype(float), f64(q), f64(bmin), f64(bmax), float(c))

    def set_problem(self, prob):
        self._prob = prob

    def setup(self):
        self._batch = QpalmBatch(self.ctx, [self._prob], self.settings)
        return self

    def warm_start(self, x=None, y=None):
        self._batch.warm_start(None if x is None else f64(x)[None, :], None if y is None else f64(y)[None, :])

    def solve(self):
        self._batch.solve()
        return self.info

    def update_settings(self, s):
        return self._batch.update_settings(s)

    def update_bounds(self, bmin=None, bmax=None):
        return self._batch.update_bounds(None if bmin is None else f64(bmin)[None, :], None if bmax is None else f64(bmax)[None, :])

    def update_q(self, q):
        self._batch.update_q(f64(q)[None, :])

    def update_Q_A(self, Qx, Ax):
        """new values of Q and A (same patterns), in the order of the problem's own Qx / Ax"""
        self._batch.update_Q_A([f64(Qx)], [f64(Ax)])

    @property
    def info(self):
        return self._batch.info(0)

    @property
    def status_val(self):
        return int(self.info.status_val)

    @property
    def x(self):
        return self._batch.solution()[0][0]

    @property
    def y(self):
        return self._batch.solution()[1][0]

    @property
    def batch(self):
        return self._batch
