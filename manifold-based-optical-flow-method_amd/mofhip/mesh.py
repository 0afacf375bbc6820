"""Device-resident mesh handle: the object the drop-in
``compute_geometrical_quantities`` returns where the reference returns its
``a2`` lil_matrix (compute_optical_flow.py:49,97).

S3 never looks inside ``a2``; it only hands it back to
``compute_velocity_field`` (S3…py:97-117). :class:`DeviceMesh` therefore
keeps a2 (and the rest of the mesh constants) in HBM and offers ``tocsr()``
for inspection and parity checks.
"""
from __future__ import annotations

import ctypes
import threading
import time

import numpy as np

from . import _lib as L


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class DeviceMesh:
    """One triangle mesh, resident on one or more GPUs (one handle each)."""

    def __init__(self, coordinates, normals, triangles, areas, device: int = 0,
                 reorder: bool = True):
        coords = np.asarray(coordinates)
        tri = np.asarray(triangles)
        if coords.ndim != 2 or coords.shape[1] != 3:
            raise ValueError("coordinates must be (N, 3)")
        if tri.ndim != 2 or tri.shape[1] != 3:
            raise ValueError("triangles must be (M, 3)")
        self.f32_points = coords.dtype == np.float32
        self._xyz = _f64(coords)
        self._nrm = _f64(normals)
        self._tri = np.ascontiguousarray(tri, dtype=np.int32)
        self._area = _f64(np.asarray(areas).reshape(-1))
        self.N = len(self._xyz)
        self.M = len(self._tri)
        if self._nrm.shape != (self.N, 3) or len(self._area) != self.M:
            raise ValueError("normals must be (N, 3) and areas (M,)")
        self.reorder = bool(reorder)  # RCM vertex order on the device (results unaffected)
        self._handles = {}
        self._locks = {}
        self._build_locks = {}
        self._glock = threading.Lock()  # guards the dicts only; builds run outside it
        self.build_seconds = {}  # wall seconds of each handle's build (per device)
        self.device = int(device)
        self.handle(self.device)

    # -- handles ---------------------------------------------------------
    def handle(self, device: int | None = None) -> ctypes.c_void_p:
        """The handle on ``device``, built on first use: the primary device's
        with ``mof_mesh_create`` (host pattern, orders, the per-mesh kernels),
        every other device's with ``mof_mesh_clone`` of it (the host state
        and multigrid hierarchy are shared, only uploads and the per-mesh
        kernels run). Builds of different devices run concurrently; only the
        same device's build is serialised."""
        device = self.device if device is None else int(device)
        h = self._handles.get(device)
        if h is not None:
            return h
        with self._glock:
            blk = self._build_locks.setdefault(device, threading.Lock())
        with blk:
            h = self._handles.get(device)
            if h is not None:
                return h
            t0 = time.perf_counter()
            h = ctypes.c_void_p()
            if device != self.device:
                src = self.handle(self.device)
                L.check(L.lib().mof_mesh_clone(src, device, ctypes.byref(h)))
            else:
                flags = ((L.MOF_GEOM_F32_POINTS if self.f32_points else 0)
                         | (0 if self.reorder else L.MOF_NO_REORDER))
                L.check(L.lib().mof_mesh_create(
                    L.ptr(self._xyz), L.ptr(self._nrm), L.ptr(self._tri), L.ptr(self._area),
                    self.N, self.M, device, flags, ctypes.byref(h)))
            with self._glock:
                self.build_seconds[device] = time.perf_counter() - t0
                self._locks[device] = threading.Lock()
                self._handles[device] = h
        return h

    def prepare(self, devices) -> dict:
        """Build the handles of ``devices`` that do not exist yet, concurrently
        (one host thread per device; ctypes releases the GIL). Returns the
        build seconds per device."""
        todo = [int(d) for d in dict.fromkeys(devices) if int(d) not in self._handles]
        if self.device in todo:  # the clones need the primary handle
            self.handle(self.device)
            todo.remove(self.device)
        errors = []

        def run(d):
            try:
                self.handle(d)
            except BaseException as exc:  # re-raised below
                errors.append(exc)

        threads = [threading.Thread(target=run, args=(d,)) for d in todo]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
        return dict(self.build_seconds)

    def prepare_solver(self, device: int | None = None, **opts):
        """Start the per-mesh setup the solves with ``opts`` need (the
        multigrid hierarchy, mof_mesh_prepare) on a host thread of the
        handle; returns at once, the next solve waits for it."""
        o = self.make_opts(**{k: v for k, v in opts.items() if k != "batch"})
        with self.lock(device):
            L.check(L.lib().mof_mesh_prepare(self.handle(device), ctypes.byref(o)))

    def sync_solver(self, device: int | None = None):
        """Wait for the setup prepare_solver started (raises its error)."""
        with self.lock(device):
            L.check(L.lib().mof_mesh_sync(self.handle(device)))

    def lock(self, device: int | None = None) -> threading.Lock:
        device = self.device if device is None else int(device)
        self.handle(device)
        return self._locks[device]

    def close(self):
        with self._glock:
            hs = list(self._handles.values())
            self._handles.clear()
        for h in hs:
            L.lib().mof_mesh_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- matrix-like view of a2 -------------------------------------------
    @property
    def shape(self):
        return (2 * self.N, 2 * self.N)

    def info(self, device: int | None = None) -> dict:
        inf = L.MofMeshInfo()
        L.check(L.lib().mof_mesh_get_info(self.handle(device), ctypes.byref(inf)))
        return {k: getattr(inf, k) for k, _ in inf._fields_}

    @property
    def nnz(self) -> int:
        return int(self.info()["nnz_struct"])

    def geometry(self):
        """``(e (N,2,3), grad_w (M,3,3), integral_wi_wj (M,2))`` host copies."""
        e = np.empty((self.N, 2, 3))
        gw = np.empty((self.M, 3, 3))
        iw = np.empty((self.M, 2))
        with self.lock():
            L.check(L.lib().mof_geometry_export(self.handle(), L.ptr(e), L.ptr(gw), L.ptr(iw)))
        return e, gw, iw

    def _csr(self, which: int, drop_zeros: bool):
        with self.lock():
            return self._csr_locked(which, drop_zeros)

    def tocsr(self, drop_zeros: bool = True):
        """a2 as scipy CSR; ``drop_zeros`` mirrors lil's zero removal."""
        return self._csr(L.MOF_CSR_A2, drop_zeros)

    def assemble(self, I0, I1, dt, lambda_, drop_zeros: bool = True):
        """One timestep's ``(A = a1 + lambda*a2 as CSR, f)`` (worker :113-146)."""
        I0 = _f64(I0)
        I1 = _f64(I1)
        if I0.shape != (self.N,) or I1.shape != (self.N,):
            raise ValueError("I0 and I1 must be (N,)")
        f = np.empty(2 * self.N)
        with self.lock():
            L.check(L.lib().mof_assemble(self.handle(), L.ptr(I0), L.ptr(I1), float(dt),
                                         float(lambda_), L.ptr(f)))
            A = self._csr_locked(L.MOF_CSR_A_LAST, drop_zeros)
        return A, f

    def _csr_locked(self, which, drop_zeros):
        import scipy.sparse as sp
        cap = self.nnz
        indptr = np.empty(2 * self.N + 1, np.int32)
        indices = np.empty(cap, np.int32)
        data = np.empty(cap)
        nnz = ctypes.c_int64(0)
        L.check(L.lib().mof_csr_export(self.handle(), which, int(bool(drop_zeros)),
                                       L.ptr(indptr), L.ptr(indices), L.ptr(data),
                                       ctypes.byref(nnz)))
        n = nnz.value
        return sp.csr_matrix((data[:n].copy(), indices[:n].copy(), indptr), shape=self.shape)

    # -- solves ------------------------------------------------------------
    @staticmethod
    def make_opts(precision="f64", batch=0, rtol=0.0, inner_rtol=0.0, max_iter=0, max_outer=0,
                  block_jacobi=True, device_io=False, time_spmv=False, stream=None,
                  precond="jacobi", recovery=True, fused=None, etol=0.0) -> L.MofOpts:
        """precond: "jacobi" (2x2 block Jacobi) or "amg" (aggregation-multigrid
        V-cycle; precision="mixed" only). recovery=False: a failed system is
        NaN-filled at once (MOF_NO_RECOVERY) instead of re-solved with block
        Jacobi and then fp64. fused (precision="f64"): True -- each batch's
        solve in one launch (MOF_SOLVE_FUSED), False -- never, None -- the
        library's choice (small meshes). etol: the refinement's error
        control -- a system also needs its estimated error below etol max|V|
        (0: the library's 1e-7, < 0: the residual test alone)."""
        o = L.MofOpts()
        o.struct_size = ctypes.sizeof(L.MofOpts)
        o.precision = {"f64": L.MOF_PREC_F64, "mixed": L.MOF_PREC_MIXED}[precision]
        o.flags = ((L.MOF_IO_DEVICE if device_io else 0)
                   | (0 if block_jacobi else L.MOF_NO_BLOCK_JACOBI)
                   | (L.MOF_TIME_SPMV if time_spmv else 0)
                   | {"jacobi": 0, "amg": L.MOF_PRECOND_AMG}[precond]
                   | (0 if recovery else L.MOF_NO_RECOVERY)
                   | {None: 0, True: L.MOF_SOLVE_FUSED, False: L.MOF_SOLVE_EAGER}[fused])
        o.batch = int(batch)
        o.max_iter = int(max_iter)
        o.max_outer = int(max_outer)
        o.rtol = float(rtol)
        o.inner_rtol = float(inner_rtol)
        o.stream = stream
        o.etol = float(etol)
        return o

    def fingerprint(self) -> str:
        """Digest of the mesh inputs (checkpoint keys, mofhip.solve)."""
        fp = getattr(self, "_fp", None)
        if fp is None:
            from .solve import _digest
            fp = self._fp = _digest(self._xyz, self._nrm, self._tri, self._area, self.f32_points)
        return fp

    def solve_range(self, I, t_k, k0, k1, lambda_, I2=None, device=None, raise_on_noconv=False, out=None,
                    **opts):
        """V for k in [k0, k1): (k1-k0, 2N) float64 host array, plus stats.
        ``out``: a C-contiguous float64 (k1-k0, 2N) array to write V into."""
        I = _f64(I)
        I2a = I if I2 is None else _f64(I2)
        tk = _f64(t_k)
        T = I.shape[0]
        if I.ndim != 2 or I.shape[1] != self.N or I2a.shape != I.shape:
            raise ValueError("I and I_2 must be (T, N)")
        if len(tk) < T:
            raise ValueError("t_k needs at least T entries")
        shape = (max(k1 - k0, 0), 2 * self.N)
        if out is None:
            V = np.empty(shape)
        else:
            if out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
                raise ValueError("out must be a C-contiguous float64 %s array" % (shape,))
            V = out
        st = L.MofStats()
        o = self.make_opts(**opts)
        h = self.handle(device)
        with self.lock(device):
            rc = L.lib().mof_solve_range(h, L.ptr(I), L.ptr(I2a), L.ptr(tk), T, int(k0), int(k1),
                                         float(lambda_), ctypes.byref(o), L.ptr(V),
                                         ctypes.byref(st))
        if rc == L.MOF_E_NOCONV and not raise_on_noconv:
            return V, st.as_dict()
        L.check(rc)
        return V, st.as_dict()

    def solve_range_device(self, I_ptr: int, I2_ptr: int, T: int, t_k, k0: int, k1: int,
                           lambda_, V_ptr: int, device=None, **opts):
        """Device-pointer form (inputs resident in HBM; used by bench.py)."""
        tk = _f64(t_k)
        st = L.MofStats()
        o = self.make_opts(device_io=True, **opts)
        h = self.handle(device)
        with self.lock(device):
            rc = L.lib().mof_solve_range(h, ctypes.c_void_p(I_ptr), ctypes.c_void_p(I2_ptr),
                                         L.ptr(tk), int(T), int(k0), int(k1), float(lambda_),
                                         ctypes.byref(o), ctypes.c_void_p(V_ptr),
                                         ctypes.byref(st))
        if rc != L.MOF_E_NOCONV:
            L.check(rc)
        return st.as_dict()

    def bench_spmv(self, precision="mixed", batch=1, reps=50, device=None):
        ms = ctypes.c_double(0)
        by = ctypes.c_double(0)
        prec = {"f64": L.MOF_PREC_F64, "mixed": L.MOF_PREC_MIXED}[precision]
        with self.lock(device):
            L.check(L.lib().mof_bench_spmv(self.handle(device), prec, int(batch), int(reps),
                                           ctypes.byref(ms), ctypes.byref(by)))
        return ms.value, by.value


def index_probe(triangles, n_vertices: int, sym: int = -1, reorder: bool = True) -> dict:
    """Host-only diagnostic (mof_index_probe): the level-0 SELL index tables
    the library builds for this triangle list -- ``sell_off``, ``col``,
    ``mir`` (position | 1 << 30 if transposed, -1 padding), the ``packed``
    words, and whether symmetric reads (``sym_used``) and the packed words
    (``packed_used``) are taken. ``sym``: 1 / 0 force symmetric / plain reads,
    -1 decides per mesh, as ``MOF_SYM_READS`` does for a handle."""
    T = np.ascontiguousarray(triangles, dtype=np.int32)
    N, M = int(n_vertices), len(T)
    flags = 0 if reorder else L.MOF_NO_REORDER
    nb, su, pu = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int32(0)
    L.check(L.lib().mof_index_probe(L.ptr(T), N, M, flags, int(sym), ctypes.byref(nb), None, None, None, None,
                                    None, None))
    off = np.zeros((N + 63) // 64 + 1, dtype=np.int32)
    col = np.zeros(nb.value, dtype=np.int32)
    mir = np.zeros(nb.value, dtype=np.int32)
    packed = np.zeros(nb.value, dtype=np.uint32)
    L.check(L.lib().mof_index_probe(L.ptr(T), N, M, flags, int(sym), ctypes.byref(nb), L.ptr(off), L.ptr(col),
                                    L.ptr(mir), L.ptr(packed), ctypes.byref(su), ctypes.byref(pu)))
    return {"sell_off": off, "col": col, "mir": mir, "packed": packed, "sym_used": bool(su.value),
            "packed_used": bool(pu.value)}


class _Hook:
    """A tests-only switch of the library, on inside the block (``_name``: its entry point)."""

    def __enter__(self):
        L.check(getattr(L.lib(), self._name)(1))
        return self

    def __exit__(self, *exc):
        L.check(getattr(L.lib(), self._name)(0))
        return False


class force_index32(_Hook):
    """Tests only (mof_test_force_index32): handles created inside the block
    keep the two 32-bit index tables where the packed words would fit."""
    _name = "mof_test_force_index32"


def _staged_probe(name: str, triangles, n_vertices: int, reorder: bool) -> dict:
    T = np.ascontiguousarray(triangles, dtype=np.int32)
    flags = 0 if reorder else L.MOF_NO_REORDER
    nb, used = ctypes.c_int64(0), ctypes.c_int32(0)
    L.check(getattr(L.lib(), name)(L.ptr(T), int(n_vertices), len(T), flags, ctypes.byref(nb), ctypes.byref(used)))
    return {"staged_bytes": int(nb.value), "staged_used": bool(used.value)}


def _staged_launches(name: str) -> dict:
    c = np.zeros(3, dtype=np.int64)
    L.check(getattr(L.lib(), name)(L.ptr(c)))
    return {"rows": int(c[0]), "staged_one": int(c[1]), "staged_multi": int(c[2])}


def residual_probe(triangles, n_vertices: int, reorder: bool = True) -> dict:
    """Host-only diagnostic (mof_residual_probe): ``staged_bytes``, the LDS
    the staged fp64 residual (k_residual_lds) needs for the widest 64-row
    slice of this triangle list -- 64 (36 a2 slots + 192 incidence slots +
    48) bytes -- and ``staged_used``, whether a handle of the mesh takes that
    kernel (the bytes fit the kernel's fixed LDS limit). The batch plays no
    part."""
    return _staged_probe("mof_residual_probe", triangles, n_vertices, reorder)


class force_residual_rows(_Hook):
    """Tests only (mof_test_force_residual_rows): handles created inside the
    block keep the row kernel k_residual_rcn where the staged one would fit."""
    _name = "mof_test_force_residual_rows"


class force_residual_trips(_Hook):
    """Tests only (mof_test_force_residual_trips): every staged residual launch
    inside the block takes the four-trip kernel of the large launches."""
    _name = "mof_test_force_residual_trips"


def residual_launches() -> dict:
    """Tests only (mof_test_residual_launches): launches so far in this process
    of the fp64 residual's row kernel (``rows``) and of the staged kernel with
    one (``staged_one``) and four (``staged_multi``) trips per wave."""
    return _staged_launches("mof_test_residual_launches")


def assembly_probe(triangles, n_vertices: int, reorder: bool = True) -> dict:
    """Host-only diagnostic (mof_assembly_probe): ``staged_bytes``, the LDS the
    staged row assembly (k_assemble_lds) needs for the widest 64-row slice of
    this triangle list -- 64 (112 incidence slots + 48 a2 slots + 48) bytes --
    and ``staged_used``, whether a handle of the mesh takes that kernel (no
    row wider than 8 blocks and the bytes fit the kernel's fixed LDS limit).
    The batch plays no part."""
    return _staged_probe("mof_assembly_probe", triangles, n_vertices, reorder)


class force_assembly_rows(_Hook):
    """Tests only (mof_test_force_assembly_rows): handles created inside the
    block keep the row kernel k_assemble_rows_rc where the staged one would fit."""
    _name = "mof_test_force_assembly_rows"


class force_assembly_trips(_Hook):
    """Tests only (mof_test_force_assembly_trips): every staged assembly launch
    inside the block takes the multi-trip kernel of the large launches."""
    _name = "mof_test_force_assembly_trips"


def assembly_launches() -> dict:
    """Tests only (mof_test_assembly_launches): launches so far in this process
    of the row assembly kernel (``rows``) and of the staged kernel with one
    (``staged_one``) and several (``staged_multi``) trips per wave."""
    return _staged_launches("mof_test_assembly_launches")


def assembly_readback(mesh: "DeviceMesh", system: int, device=None) -> dict:
    """Tests only (mof_test_assembly_readback): what the handle's last
    mixed-precision assembly left for its system ``system``, in the internal
    order -- ``A32`` (sell_blocks, 4) float32, ``A0h`` (sell_blocks,) uint64
    (the multigrid's bf16 blocks; None without multigrid storage) and ``rhs``
    (N, 2) float64. Positions the assembly never writes are not initialised."""
    nb = int(mesh.info(device)["sell_blocks"])
    A32 = np.zeros((nb, 4), dtype=np.float32)
    A0h = np.zeros(nb, dtype=np.uint64)
    rhs = np.zeros((mesh.N, 2), dtype=np.float64)
    have = ctypes.c_int32(0)
    with mesh.lock(device):
        L.check(L.lib().mof_test_assembly_readback(mesh.handle(device), int(system), L.ptr(A32), L.ptr(A0h),
                                                   L.ptr(rhs), ctypes.byref(have)))
    return {"A32": A32, "A0h": A0h if have.value else None, "rhs": rhs}


GALERKIN_KERNELS = ("galerkin0_ns", "galerkin0_ent", "galerkin_sys2_f32", "galerkin_sys2_bf16", "galerkin_sys3",
                    "galerkin3_ns", "galerkin3_ent", "galerkin3_big")


class force_galerkin_ns:
    """Tests only (mof_test_force_galerkin_ns): multigrid setups inside the
    block take the per-position Galerkin products k_galerkin_ns<2> /
    k_galerkin_ns<3> where the by-entry ones would run."""

    def __enter__(self):
        L.check(L.lib().mof_test_force_galerkin_ns(1))
        return self

    def __exit__(self, *exc):
        L.check(L.lib().mof_test_force_galerkin_ns(0))
        return False


def galerkin_launches() -> dict:
    """Tests only (mof_test_galerkin_launches): launches so far in this process
    of each Galerkin product kernel (``GALERKIN_KERNELS``)."""
    c = np.zeros(len(GALERKIN_KERNELS), dtype=np.int64)
    L.check(L.lib().mof_test_galerkin_launches(L.ptr(c)))
    return {k: int(v) for k, v in zip(GALERKIN_KERNELS, c)}


def amg_levels(mesh: "DeviceMesh", device=None) -> dict:
    """Tests only (mof_test_amg_levels): the host multigrid hierarchy the
    handle's preconditioner was built from (after a multigrid solve), as
    ``{"regular", "omega", "omega1", "nc", "cap", "levels": [...]}``; each level
    a dict of ``n, bs, sell_nb, smoothed, sym, has_Ah, packed`` (the device keeps
    the level's fp32 operator packed: diagonal and upper blocks, 9 floats each) and the arrays
    ``sell_off, sell_col, sell_row, diag_pos``, level 0 ``mirror``, levels >= 1
    ``dead`` (n, 3) and ``twin``, and for the transition to the next level
    ``agg, pptr, pcol, Q`` (P blocks, bs, 3), ``gptr, gent`` (terms, 3)."""
    f = L.lib().mof_test_amg_levels
    nl = ctypes.c_int32(0)
    om = np.zeros(2, dtype=np.float32)
    none = [None] * 13
    out = {"levels": []}
    with mesh.lock(device):
        h = mesh.handle(device)
        L.check(f(h, -1, ctypes.byref(nl), None, L.ptr(om), *none))
        for l in range(nl.value):
            sz = np.zeros(16, dtype=np.int64)
            L.check(f(h, l, ctypes.byref(nl), L.ptr(sz), None, *none))
            n, bs, nb = int(sz[0]), int(sz[1]), int(sz[2])
            i32 = lambda k: np.zeros(int(k), dtype=np.int32)  # noqa: E731
            lv = {"n": n, "bs": bs, "sell_nb": nb, "smoothed": bool(sz[4]), "sym": bool(sz[12]),
                  "has_Ah": bool(sz[15] & 1), "packed": bool(sz[15] & 2), "sell_off": i32(sz[3]), "sell_col": i32(nb), "sell_row": i32(nb),
                  "diag_pos": i32(n), "dead": np.zeros((n, 3) if l else (0, 3), dtype=np.uint8),
                  "twin": i32(nb if l else 0), "mirror": i32(0 if l else nb), "agg": i32(sz[5]), "pptr": i32(sz[6]),
                  "pcol": i32(sz[7]), "Q": np.zeros((int(sz[8]) // (3 * bs), bs, 3), dtype=np.float32),
                  "gptr": i32(sz[9]), "gent": np.zeros((int(sz[10]) // 3, 3), dtype=np.int32)}
            p = lambda k: L.ptr(lv[k]) if lv[k].size else None  # noqa: E731
            L.check(f(h, l, ctypes.byref(nl), None, None, p("sell_off"), p("sell_col"), p("sell_row"), p("diag_pos"),
                      p("dead"), p("twin"), p("mirror"), p("agg"), p("pptr"), p("pcol"), p("Q"), p("gptr"),
                      p("gent")))
            out["levels"].append(lv)
            out.update(regular=bool(sz[11]), nc=int(sz[13]), cap=int(sz[14]))
    out.update(omega=float(om[0]), omega1=float(om[1]))
    return out


def amg_readback(mesh: "DeviceMesh", level: int, system: int, n: int, sell_nb: int, has_Ah: bool, nc: int = 0,
                 device=None) -> dict:
    """Tests only (mof_test_amg_readback): what the handle's last multigrid
    setup left for ``system`` on coarse level ``level`` (its ``n``, ``sell_nb``
    and ``has_Ah`` from ``amg_levels``): ``A`` (sell_nb, 3, 4) float32 (a packed
    level's blocks widened on the host, each lower block its upper twin transposed), ``Dh``
    (n, 4) uint32 and ``Dh22`` (n,) uint16, with ``has_Ah`` the sweep copy ``Ah``
    (sell_nb, 2) uint32 and ``Ah22`` (sell_nb, 2) uint16, and with ``nc`` > 0 (the
    coarsest level) ``cinv`` (nc, nc) float32."""
    r = {"A": np.zeros((sell_nb, 3, 4), dtype=np.float32), "Dh": np.zeros((n, 4), dtype=np.uint32),
         "Dh22": np.zeros(n, dtype=np.uint16)}
    if has_Ah:
        r["Ah"] = np.zeros((sell_nb, 2), dtype=np.uint32)
        r["Ah22"] = np.zeros((sell_nb, 2), dtype=np.uint16)
    if nc:
        r["cinv"] = np.zeros((nc, nc), dtype=np.float32)
    p = lambda k: L.ptr(r[k]) if k in r else None  # noqa: E731
    with mesh.lock(device):
        L.check(L.lib().mof_test_amg_readback(mesh.handle(device), int(level), int(system), p("A"), p("Dh"),
                                              p("Dh22"), p("Ah"), p("Ah22"), p("cinv")))
    return r


VCYCLE_KERNELS = ("res0_ns", "res0_ns_pk", "restrict2", "restrict3", "restrict0_sa2", "restrict0_sa3", "res3",
                  "subcycle", "prolong3", "prolong3_sa", "prolong0_x1", "prolong0_x2", "prolong0_sa_x1",
                  "prolong0_sa_x2", "post3", "bsweep_h", "bsweep_f") + tuple(
    "post0_x%d_%s%s" % (xm, "zh" if zh else "zf", "_pk" if pk else "")
    for xm in (1, 2) for zh in (0, 1) for pk in (0, 1))


def vcycle_launches() -> dict:
    """Tests only (mof_test_vcycle_launches): launches so far in this process
    of each V-cycle kernel instance (``VCYCLE_KERNELS``; ``post0_x<XM>_<zh|zf>[_pk]``
    are k_post0_ns's eight)."""
    c = np.zeros(len(VCYCLE_KERNELS), dtype=np.int64)
    L.check(L.lib().mof_test_vcycle_launches(L.ptr(c)))
    return {k: int(v) for k, v in zip(VCYCLE_KERNELS, c)}


def amg_vcycle_tables(mesh: "DeviceMesh", n_levels: int, system: int = 0, device=None) -> dict:
    """Tests only (mof_test_amg_vcycle_tables): ``xm``, ``zh`` (the mesh's own
    choice), ``S`` (the first level inside k_subcycle), ``nblk``, per level
    ``apos, mptr, mlist, rptr, rent`` (``levels``), and on a handle with
    boundary sweeps ``bsw_rows``, ``bsw_sweeps``, ``bsw_bsrc`` and ``bsw_A``
    (slots, 2) uint32, the ring blocks of ``system``."""
    f = L.lib().mof_test_amg_vcycle_tables
    out = {"levels": []}
    none = [None] * 8
    with mesh.lock(device):
        h = mesh.handle(device)
        for l in range(n_levels):
            sz = np.zeros(12, dtype=np.int64)
            L.check(f(h, l, int(system), L.ptr(sz), *none))
            t = {k: np.zeros(int(sz[i]), dtype=np.int32) for i, k in enumerate(("apos", "mptr", "mlist", "rptr", "rent"))}
            p = lambda k: L.ptr(t[k]) if t[k].size else None  # noqa: E731
            L.check(f(h, l, int(system), None, p("apos"), p("mptr"), p("mlist"), p("rptr"), p("rent"), None, None, None))
            t["rent"] = t["rent"].reshape(-1, 2)
            out["levels"].append(t)
        out.update(xm=int(sz[5]), zh=bool(sz[6]), S=int(sz[7]), bsw_n=int(sz[8]), bsw_sweeps=int(sz[9]),
                   nblk=int(sz[11]))
        if out["bsw_n"]:
            out["bsw_rows"] = np.zeros(int(sz[8]), dtype=np.int32)
            out["bsw_bsrc"] = np.zeros(int(sz[10]), dtype=np.int32)
            out["bsw_A"] = np.zeros((int(sz[10]), 2), dtype=np.uint32)
            L.check(f(h, 0, int(system), None, None, None, None, None, None, L.ptr(out["bsw_rows"]),
                      L.ptr(out["bsw_bsrc"]), L.ptr(out["bsw_A"])))
    return out


def amg_vcycle(mesh: "DeviceMesh", r, level_sizes, systems=(), smap=None, retired=None, zh=None, tap=False,
               sentinel=None, device=None) -> dict:
    """Tests only (mof_test_amg_vcycle): the production V-cycle of the handle's
    last multigrid batch applied to ``r`` (B, N, 2) float32 in the internal
    order, over the systems ``smap`` lists (all B without) except those flagged
    in ``retired`` (B,); ``zh`` forces z's format (None: the mesh's own);
    ``tap`` keeps level 0's iterate at four points; ``sentinel`` is the word
    the cycle's outputs are filled with beforehand. ``level_sizes``: every
    level's ``n`` (amg_levels). Returns ``zh, xm, S, nblk``, ``z_words`` (B, N
    [, 2]) uint32, ``z`` (B, N, 2) float32 decoded, ``rz`` (B,), and per system
    read back ``r1`` (N,) uint32, ``taps`` (level 0's iterate on entry, after
    the pre-sweep, after the prolongation, after the post-sweep: (N,) uint32
    in the bf16 pair format, the last two (N, 2) float32 words with xm = 2;
    empty without ``tap``) and ``coarse``: per level >= 1 a dict of ``b, x, r,
    y`` (n, 4) float32: the device's 12-byte rows and a fourth word, 0 or, on a
    row that still holds the sentinel, the sentinel."""
    r = np.ascontiguousarray(r, dtype=np.float32)
    B, N = r.shape[0], r.shape[1]
    assert r.shape == (B, N, 2)
    systems = np.ascontiguousarray(systems, dtype=np.int32)
    ns = len(systems)
    per = sum(16 * int(n) for n in level_sizes[1:])
    z = np.zeros((B, N, 2), dtype=np.uint32)
    rz = np.zeros(B, dtype=np.float64)
    r1 = np.zeros((ns, N), dtype=np.uint32)
    taps = np.zeros((ns, 4, N, 2), dtype=np.uint32)
    coarse = np.zeros((ns, per), dtype=np.float32)
    meta = np.zeros(4, dtype=np.int32)
    sm = None if smap is None else np.ascontiguousarray(smap, dtype=np.int32)
    rt = None if retired is None else np.ascontiguousarray(retired, dtype=np.uint8)
    assert rt is None or rt.shape == (B,)
    sw = None if sentinel is None else np.array([sentinel], dtype=np.uint32)
    o = lambda a: None if a is None else L.ptr(a)  # noqa: E731
    with mesh.lock(device):
        L.check(L.lib().mof_test_amg_vcycle(mesh.handle(device), B, L.ptr(r), o(sm), 0 if sm is None else len(sm), o(rt),
                                            -1 if zh is None else int(bool(zh)), int(bool(tap)), o(sw), L.ptr(z),
                                            L.ptr(rz), ns, o(systems) if ns else None, L.ptr(r1), L.ptr(taps),
                                            L.ptr(coarse), L.ptr(meta)))
    out = {"zh": bool(meta[0]), "xm": int(meta[1]), "S": int(meta[2]), "nblk": int(meta[3]), "rz": rz, "sys": {}}
    if out["zh"]:
        w = z.reshape(-1)[:B * N].reshape(B, N)
        out["z_words"] = w.copy()
        out["z"] = np.stack([(w << np.uint32(16)).view(np.float32), (w & np.uint32(0xFFFF0000)).view(np.float32)], axis=-1)
    else:
        out["z_words"] = z
        out["z"] = z.view(np.float32)
    for k, s in enumerate(systems):
        lev, q = [None], 0
        for n in level_sizes[1:]:
            d = {}
            for name in ("b", "x", "r", "y"):
                d[name] = coarse[k, q:q + 4 * n].reshape(n, 4).copy()
                q += 4 * n
            lev.append(d)
        # a tap in the bf16 pair format fills the first N words of its slot
        tp = [taps[k, t].copy() if t >= 2 and out["xm"] == 2 else taps[k, t].reshape(-1)[:N].copy()
              for t in range(4)] if tap else []
        out["sys"][int(s)] = {"r1": r1[k].copy(), "taps": tp, "coarse": lev}
    return out


PCG_KERNELS = tuple("spmv_%s%s%s%s" % (v, "_first" if first else "", "_zh" if zh else "", "_pk" if pk else "")
                    for v in ("f32", "f64") for first in (0, 1) for zh in (0, 1) for pk in (0, 1)) + (
    "red_pq", "red_rzrr", "update", "conv_early", "outer_update", "outer_check", "compact")
SYS_I = ("CONV", "ACTIVE", "FAILED", "ITSUM", "BEST_IT", "FAIL_IT", "FAIL_WHY", "ITMAX", "MET")
SYS_D = ("TOL2", "RR", "FF", "REL", "RR0", "BEST", "OUTER", "EST", "XMAX")
SYS_STRIDE = 12


def pcg_launches() -> dict:
    """Tests only (mof_test_pcg_launches): launches so far in this process of
    each inner-PCG kernel instance (``PCG_KERNELS``; ``spmv_<f32|f64>[_first][_zh][_pk]``
    are k_pcg_spmv's; the f64 ones exist without ``_zh`` / ``_pk`` only; ``compact``:
    the times pcg() switched to a compacted system map)."""
    c = np.zeros(len(PCG_KERNELS), dtype=np.int64)
    L.check(L.lib().mof_test_pcg_launches(L.ptr(c)))
    return {k: int(v) for k, v in zip(PCG_KERNELS, c)}


def _sys_rows(si, sd):
    out = {k: si[:, i].copy() for i, k in enumerate(SYS_I)}
    out.update({k: sd[:, i].copy() for i, k in enumerate(SYS_D)})
    return out


def pcg_inner(mesh: "DeviceMesh", rhs, rtol, cap, precond="jacobi", precision="mixed", outer_rtol=0.0, etol=0.0,
              active=None, hint=None, sentinel=None, a_system=-1, device=None) -> dict:
    """Tests only (mof_test_pcg_inner): the production inner PCG of the
    handle's last batch on ``rhs`` (B, N, 2) float64 in the internal order,
    capped at ``cap`` iterations. ``active`` (B,) selects the systems to run,
    ``hint`` = (first chunk, bulk hint) as pcg() keeps them, ``sentinel`` the
    word the vectors are filled with beforehand. Returns the vectors ``x, r, p,
    q`` (B, N, 2) in the working type, ``z`` (B, N, 2) decoded and ``z_words``,
    ``x0_words`` (B, N) with the multigrid, ``scal`` (2 slots, B, 3: r.z, |r|^2,
    p.q), ``sys`` (the sysi / sysd rows by name), ``dinv`` (B, N, 2, 2) with
    block Jacobi, ``A`` (sell_blocks, 2, 2) of ``a_system``, ``hint`` after the
    solve and ``zh, sym, packed, selfred, nblk, iterations, slowest``."""
    rhs = np.ascontiguousarray(rhs, dtype=np.float64)
    B, N = rhs.shape[0], rhs.shape[1]
    assert rhs.shape == (B, N, 2) and N == mesh.N
    amg = {"jacobi": 0, "amg": 1}[precond]
    dt = {"mixed": np.float32, "f64": np.float64}[precision]
    wt = {"mixed": np.uint32, "f64": np.uint64}[precision]
    vec = {k: np.zeros((B, N, 2), dtype=wt) for k in "xrzpq"}
    x0 = np.zeros((B, N), dtype=np.uint32)
    scal = np.zeros((2, B, 3), dtype=np.float64)
    si = np.zeros((B, SYS_STRIDE), dtype=np.int32)
    sd = np.zeros((B, SYS_STRIDE), dtype=np.float64)
    dinv = np.zeros((B, N, 2, 2), dtype=dt)
    nb = int(mesh.info(device)["sell_blocks"])
    A = np.zeros((nb, 2, 2), dtype=dt)
    meta = np.zeros(8, dtype=np.int32)
    act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
    assert act is None or act.shape == (B,)
    hn = np.zeros(2, dtype=np.int32) if hint is None else np.ascontiguousarray(hint, dtype=np.int32).copy()
    sw = None if sentinel is None else np.array([sentinel], dtype=np.uint32)
    o = lambda a: None if a is None else L.ptr(a)  # noqa: E731
    with mesh.lock(device):
        L.check(L.lib().mof_test_pcg_inner(
            mesh.handle(device), B, L.ptr(rhs), float(rtol), float(outer_rtol), float(etol), amg,
            {"mixed": L.MOF_PREC_MIXED, "f64": L.MOF_PREC_F64}[precision], int(cap), o(act), L.ptr(hn), o(sw),
            L.ptr(vec["x"]), L.ptr(vec["r"]), L.ptr(vec["z"]), L.ptr(vec["p"]), L.ptr(vec["q"]), L.ptr(x0),
            L.ptr(scal), L.ptr(si), L.ptr(sd), L.ptr(dinv), int(a_system), L.ptr(A), L.ptr(meta)))
    assert meta[7] == SYS_STRIDE
    out = {k: vec[k].view(dt) for k in "xrpq"}
    out["words"] = vec
    zh = bool(meta[0])
    if zh:
        w = vec["z"].reshape(-1)[:B * N].reshape(B, N).copy()
        out["z_words"] = w
        out["z"] = np.stack([(w << np.uint32(16)).view(np.float32), (w & np.uint32(0xFFFF0000)).view(np.float32)], axis=-1)
    else:
        out["z_words"] = vec["z"]
        out["z"] = vec["z"].view(dt)
    out.update(x0_words=x0 if amg else None, scal=scal, sys=_sys_rows(si, sd), dinv=None if amg else dinv,
               A=A if a_system >= 0 else None, hint=(int(hn[0]), int(hn[1])), zh=zh, sym=bool(meta[1]),
               packed=bool(meta[2]), selfred=bool(meta[3]), nblk=int(meta[4]), iterations=int(meta[5]),
               slowest=int(meta[6]))
    return out


def outer_readback(mesh: "DeviceMesh", B: int, precision="mixed", device=None) -> dict:
    """Tests only (mof_test_outer_readback): what the handle's last solve of a
    batch of ``B`` left -- ``x64``, ``r64`` (B, N, 2), the last inner solve's x
    ``xin`` (B, N, 2) in the working type of ``precision`` and ``sys`` (the
    sysi / sysd rows by name)."""
    N = mesh.N
    x64 = np.zeros((B, N, 2))
    r64 = np.zeros((B, N, 2))
    xin = np.zeros((B, N, 2), dtype={"mixed": np.float32, "f64": np.float64}[precision])
    si = np.zeros((B, SYS_STRIDE), dtype=np.int32)
    sd = np.zeros((B, SYS_STRIDE), dtype=np.float64)
    with mesh.lock(device):
        L.check(L.lib().mof_test_outer_readback(mesh.handle(device), int(B), L.ptr(x64), L.ptr(r64), L.ptr(xin),
                                                xin.itemsize, L.ptr(si), L.ptr(sd)))
    return {"x64": x64, "r64": r64, "xin": xin, "sys": _sys_rows(si, sd)}
