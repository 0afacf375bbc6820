"""Domain-decomposed solve: one timestep's system
split over P vertex parts, PCG iterations in lockstep with a halo exchange.

Timestep shards (:mod:`mofhip.solve`) stay the throughput path; this is the
path for a mesh one GPU should not hold alone, or for the latency of a single
timestep. Two transports (include/mof.h, ``mof_dd_*``):

* :class:`DecomposedMesh` -- all P parts in this process on one device
  (in-process halo gather, shared partial sums);
* :class:`DecomposedMesh` with ``group=`` -- one part per rank of a
  ``torch.distributed`` job (one process per GPU), halo and scalar reductions
  over RCCL; rank 0 makes the RCCL id and ``group`` broadcasts it;
* the same with ``transport="host"`` -- the per-rank plans and pack / unpack
  kernels of the RCCL transport, every exchange staged through host memory
  and carried by ``group`` itself (gloo): no RCCL, and ranks may share a GPU.

Both return V in the reference's planar layout and caller order, like
:meth:`DeviceMesh.solve_range` (compute_optical_flow.py:147, :190-191).
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np

from . import _lib as L
from .mesh import DeviceMesh, _f64


def partition_rcb(coordinates, nparts: int) -> np.ndarray:
    """Recursive coordinate bisection: (N,) part id per vertex (host)."""
    xyz = _f64(coordinates)
    part = np.empty(len(xyz), np.int32)
    L.check(L.lib().mof_partition_rcb(L.ptr(xyz), len(xyz), int(nparts), L.ptr(part)))
    return part


def plan_info(triangles, N: int, part) -> dict:
    """Per-part halo plan of a vertex partition (host): owned, ghost,
    neighbour, local-triangle and send-row counts."""
    tri = np.ascontiguousarray(triangles, dtype=np.int32)
    part = np.ascontiguousarray(part, dtype=np.int32)
    P = int(part.max()) + 1 if len(part) else 0
    out = {k: np.empty(P, np.int32) for k in ("n_own", "n_ghost", "n_nbr", "n_tri")}
    out["n_send"] = np.empty(P, np.int64)
    L.check(L.lib().mof_dd_plan_info(L.ptr(tri), int(N), len(tri), P, L.ptr(part),
                                     L.ptr(out["n_own"]), L.ptr(out["n_ghost"]),
                                     L.ptr(out["n_nbr"]), L.ptr(out["n_tri"]),
                                     L.ptr(out["n_send"])))
    return out


class HostTransport:
    """mof_dd_transport over a torch.distributed group (gloo, CPU tensors):
    the all-gather of partial records / owned V and the neighbour exchange of
    packed halo segments, called from inside the solver loop.

    Errors end the solve on every rank, not only on the rank that saw them:
    a local failure inside an exchange (copying a segment in or out) still
    completes that exchange's sends and receives with placeholder bytes, and
    every all-gather carries a status byte, so the next all-gather (the solver
    runs one after every exchange) returns failure on all ranks at the same
    call. A failure of the transport itself (a peer gone) can only end at the
    process group's timeout: create the group with a short ``timeout`` for
    this transport."""

    def __init__(self, group=None):
        import torch
        import torch.distributed as dist
        self._dist, self._torch, self.group = dist, torch, group
        self.world = dist.get_world_size(group)
        self._failed = False  # a local error waiting to be reported to every rank
        self._ag = L.ALLGATHER_FN(self._allgather)
        self._ex = L.EXCHANGE_FN(self._exchange)
        self.struct = L.MofDdTransport(None, self._ag, self._ex)

    def _peer(self, r):
        g = self.group
        if g is None or not hasattr(self._dist, "get_global_rank"):
            return int(r)
        return self._dist.get_global_rank(g, int(r))

    def _allgather(self, ctx, send, recv, nbytes):
        t = self._torch
        try:
            src = t.zeros(nbytes + 1, dtype=t.uint8)
            try:
                src[1:] = t.frombuffer(bytearray(ctypes.string_at(send, nbytes)), dtype=t.uint8)
            except Exception:
                self._failed = True
            src[0] = 1 if self._failed else 0
            out = [t.empty(nbytes + 1, dtype=t.uint8) for _ in range(self.world)]
            self._dist.all_gather(out, src, group=self.group)
        except Exception:  # the transport itself failed
            return 1
        if any(int(o[0]) for o in out):
            self._failed = False
            return 1  # some rank failed: every rank reports it at this call
        try:
            for r, o in enumerate(out):
                ctypes.memmove(recv + r * nbytes, o.data_ptr() + 1, nbytes)
        except Exception:
            return 1  # local only, after the collective: the peers are not blocked
        return 0

    def _exchange(self, ctx, n, peers, send, sbytes, recv, rbytes):
        t = self._torch
        try:
            reqs, bufs = [], []
            for k in range(n):
                if sbytes[k]:
                    try:
                        st = t.frombuffer(bytearray(ctypes.string_at(send[k], sbytes[k])), dtype=t.uint8)
                    except Exception:
                        self._failed = True
                        st = t.zeros(sbytes[k], dtype=t.uint8)
                    reqs.append(self._dist.isend(st, self._peer(peers[k]), group=self.group))
                if rbytes[k]:
                    rt = t.empty(rbytes[k], dtype=t.uint8)
                    bufs.append((k, rt))
                    reqs.append(self._dist.irecv(rt, self._peer(peers[k]), group=self.group))
            for q in reqs:
                q.wait()
        except Exception:  # the transport itself failed
            return 1
        try:
            for k, rt in bufs:
                ctypes.memmove(recv[k], rt.data_ptr(), rbytes[k])
        except Exception:
            self._failed = True
        return 0


class DecomposedMesh:
    """One mesh decomposed into ``nparts`` vertex parts (RCB unless ``part``
    is given). Without ``group`` every part lives in this process on
    ``device``; with a torch.distributed ``group`` this rank drives part
    ``group.rank()`` on ``device`` and ``nparts`` must equal the group size.
    ``staged`` (in-process only): exchange through the pack / copy / unpack
    kernels of the RCCL transport (a one-GPU rehearsal of that path).
    ``transport`` (with ``group``): "rccl" (default) or "host" (host-staged
    exchanges over ``group``, see :class:`HostTransport`)."""

    def __init__(self, coordinates, normals, triangles, areas, nparts: int, device: int = 0,
                 part=None, group=None, rank=None, staged: bool = False, transport: str = "rccl"):
        coords = np.asarray(coordinates)
        tri = np.asarray(triangles)
        if coords.ndim != 2 or coords.shape[1] != 3 or tri.ndim != 2 or tri.shape[1] != 3:
            raise ValueError("coordinates must be (N, 3) and triangles (M, 3)")
        self.f32_points = coords.dtype == np.float32
        self._xyz = _f64(coords)
        self._nrm = _f64(normals)
        self._tri = np.ascontiguousarray(tri, dtype=np.int32)
        self._area = _f64(np.asarray(areas).reshape(-1))
        self.N = len(self._xyz)
        self.M = len(self._tri)
        if self._nrm.shape != (self.N, 3) or len(self._area) != self.M:
            raise ValueError("normals must be (N, 3) and areas (M,)")
        self.nparts = int(nparts)
        self._part = None if part is None else np.ascontiguousarray(part, dtype=np.int32)
        if self._part is not None and self._part.shape != (self.N,):
            raise ValueError("part must be (N,)")
        self.device = int(device)
        flags = ((L.MOF_GEOM_F32_POINTS if self.f32_points else 0)
                 | (L.MOF_DD_STAGED if staged else 0))
        h = ctypes.c_void_p()
        pp = L.ptr(self._part) if self._part is not None else None
        if group is None:
            L.check(L.lib().mof_dd_create(L.ptr(self._xyz), L.ptr(self._nrm), L.ptr(self._tri),
                                          L.ptr(self._area), self.N, self.M, self.nparts, pp,
                                          self.device, flags, ctypes.byref(h)))
        else:
            import torch.distributed as dist
            r = dist.get_rank(group) if rank is None else int(rank)
            if dist.get_world_size(group) != self.nparts:
                raise ValueError("nparts must equal the group size (one part per rank)")
            if transport == "host":
                self._transport = HostTransport(group)
                L.check(L.lib().mof_dd_create_rank_host(
                    L.ptr(self._xyz), L.ptr(self._nrm), L.ptr(self._tri), L.ptr(self._area), self.N, self.M,
                    self.nparts, pp, r, ctypes.byref(self._transport.struct), self.device, flags,
                    ctypes.byref(h)))
                self._h = h
                return
            if transport != "rccl":
                raise ValueError("transport must be 'rccl' or 'host'")
            ident = np.zeros(L.MOF_DD_ID_BYTES, np.uint8)
            if r == 0:
                L.check(L.lib().mof_dd_unique_id(L.ptr(ident)))
            box = [ident.tobytes()]
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if hasattr(
                dist, "get_global_rank") else 0, group=group)
            ident = np.frombuffer(box[0], np.uint8).copy()
            L.check(L.lib().mof_dd_create_rank(L.ptr(self._xyz), L.ptr(self._nrm),
                                               L.ptr(self._tri), L.ptr(self._area), self.N,
                                               self.M, self.nparts, pp, r, L.ptr(ident),
                                               self.device, flags, ctypes.byref(h)))
        self._h = h

    def info(self) -> dict:
        inf = L.MofDdInfo()
        L.check(L.lib().mof_dd_get_info(self._h, ctypes.byref(inf)))
        return {k: getattr(inf, k) for k, _ in inf._fields_ if k != "pad_"}

    def close(self):
        if getattr(self, "_h", None):
            L.lib().mof_dd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve_range(self, I, t_k, k0, k1, lambda_, I2=None, raise_on_noconv=False, **opts):
        """V for k in [k0, k1): (k1-k0, 2N) float64 host array, plus stats
        (options as :meth:`DeviceMesh.make_opts`; precond "amg" = a multigrid
        V-cycle per part on its owned rows, block Jacobi across the parts)."""
        I = _f64(I)
        I2a = I if I2 is None else _f64(I2)
        tk = _f64(t_k)
        T = I.shape[0]
        if I.ndim != 2 or I.shape[1] != self.N or I2a.shape != I.shape:
            raise ValueError("I and I_2 must be (T, N)")
        if len(tk) < T:
            raise ValueError("t_k needs at least T entries")
        V = np.empty((max(k1 - k0, 0), 2 * self.N))
        st = L.MofStats()
        o = DeviceMesh.make_opts(**opts)
        rc = L.lib().mof_dd_solve_range(self._h, L.ptr(I), L.ptr(I2a), L.ptr(tk), T, int(k0),
                                        int(k1), float(lambda_), ctypes.byref(o), L.ptr(V),
                                        ctypes.byref(st))
        if rc == L.MOF_E_NOCONV and not raise_on_noconv:
            return V, st.as_dict()
        L.check(rc)
        return V, st.as_dict()

    def solve_range_device(self, I_ptr: int, I2_ptr: int, T: int, t_k, k0: int, k1: int,
                           lambda_, V_ptr: int, **opts):
        """Device-pointer form (inputs resident in HBM; bench.py)."""
        tk = _f64(t_k)
        st = L.MofStats()
        o = DeviceMesh.make_opts(device_io=True, **opts)
        rc = L.lib().mof_dd_solve_range(self._h, ctypes.c_void_p(I_ptr), ctypes.c_void_p(I2_ptr),
                                        L.ptr(tk), int(T), int(k0), int(k1), float(lambda_),
                                        ctypes.byref(o), ctypes.c_void_p(V_ptr),
                                        ctypes.byref(st))
        if rc != L.MOF_E_NOCONV:
            L.check(rc)
        return st.as_dict()


# ---- test hooks (include/mof.h, mof_dd_test_*) ---------------------------------------

DD_KERNELS = ("halo_pull_f32", "halo_pull_f64", "halo_pack_f32", "halo_pack_f64", "halo_unpack_f32",
              "halo_unpack_f64", "dd_scatter", "dd_own_pack", "dd_own_scatter")


def dd_launches() -> dict:
    """Tests only (mof_dd_test_launches): launches so far in this process of
    each halo / gather kernel instance (``DD_KERNELS``)."""
    c = np.zeros(len(DD_KERNELS), dtype=np.int64)
    L.check(L.lib().mof_dd_test_launches(L.ptr(c)))
    return {k: int(v) for k, v in zip(DD_KERNELS, c)}


class PartHandle:
    """Tests only (mof_dd_test_part): local part ``l`` of a DecomposedMesh --
    its plan (``part, n_own, n_ghost, n_tri, l2g, ghost_owner, ghost_src, nbr,
    recv_off, send_off, send_idx``) and its borrowed mesh handle, with the
    ``N / handle / lock / info`` the test hooks of :mod:`mofhip.mesh` take of a
    DeviceMesh. Valid while the DecomposedMesh is open."""

    def __init__(self, dd: "DecomposedMesh", l: int):
        f = L.lib().mof_dd_test_part
        h = ctypes.c_void_p()
        sz = np.zeros(12, dtype=np.int64)
        L.check(f(dd._h, int(l), ctypes.byref(h), L.ptr(sz), *([None] * 7)))
        self._dd, self._handle, self._lock = dd, h, threading.Lock()
        self.part, self.n_own, self.n_ghost, nn, ns, self.n_tri = (int(v) for v in sz[:6])
        self.nparts, self.local_parts, self.n_halo, self.cap, self.nmax, self.nmax_own = (int(v) for v in sz[6:12])
        self.N = self.n_own + self.n_ghost
        i32 = lambda n: np.zeros(max(int(n), 1), dtype=np.int32)  # noqa: E731
        a = {"l2g": i32(self.N), "ghost_owner": i32(self.n_ghost), "ghost_src": i32(self.n_ghost), "nbr": i32(nn),
             "recv_off": i32(nn + 1), "send_off": i32(nn + 1), "send_idx": i32(ns)}
        L.check(f(dd._h, int(l), None, None, *(L.ptr(a[k]) for k in a)))
        n = {"l2g": self.N, "ghost_owner": self.n_ghost, "ghost_src": self.n_ghost, "nbr": nn, "recv_off": nn + 1,
             "send_off": nn + 1, "send_idx": ns}
        for k, v in a.items():
            setattr(self, k, v[:n[k]].copy())

    def handle(self, device=None):
        return self._handle

    def lock(self, device=None):
        return self._lock

    def info(self, device=None) -> dict:
        inf = L.MofMeshInfo()
        L.check(L.lib().mof_mesh_get_info(self._handle, ctypes.byref(inf)))
        return {k: getattr(inf, k) for k, _ in inf._fields_}


def dd_parts(dd: "DecomposedMesh") -> list:
    """Tests only: the PartHandle of every local part."""
    first = PartHandle(dd, 0)
    return [first] + [PartHandle(dd, l) for l in range(1, first.local_parts)]


def _cat(vecs, dtype):
    return np.ascontiguousarray(np.concatenate([np.ascontiguousarray(v, dtype=dtype).ravel() for v in vecs]))


def _split(flat, parts, B, per=2):
    out, q = [], 0
    for p in parts:
        n = B * p.N * per
        out.append(flat[q:q + n].reshape(B, p.N, per).copy())
        q += n
    return out


def dd_halo(dd: "DecomposedMesh", parts, vecs, which: int, f32: bool, sentinel=None) -> list:
    """Tests only (mof_dd_test_halo): the production halo exchange on ``vecs``
    (one (B, n_loc, 2) array per part) put into every part's z (``which`` 0;
    float32 with ``f32``) or x64 (``which`` 1); returns the vectors after it.
    ``sentinel``: the word the staging buffers are filled with beforehand."""
    dt = np.float32 if f32 else np.float64
    B = vecs[0].shape[0]
    assert all(v.shape == (B, p.N, 2) for v, p in zip(vecs, parts))
    src = _cat(vecs, dt)
    out = np.zeros_like(src)
    sw = None if sentinel is None else np.array([sentinel], dtype=np.uint32)
    L.check(L.lib().mof_dd_test_halo(dd._h, B, int(which), int(bool(f32)), L.ptr(src), L.ptr(out),
                                     None if sw is None else L.ptr(sw)))
    return _split(out, parts, B)


def dd_gather(dd: "DecomposedMesh", parts, x64, failed=None, prefill=None) -> np.ndarray:
    """Tests only (mof_dd_test_gather): the production gather of V (B, 2 N)
    from ``x64`` (one (B, n_loc, 2) array per part) and the per-system
    ``failed`` flags; ``prefill``: the 64-bit word V holds beforehand."""
    B = x64[0].shape[0]
    assert all(v.shape == (B, p.N, 2) for v, p in zip(x64, parts))
    src = _cat(x64, np.float64)
    V = np.zeros((B, 2 * dd.N))
    fl = None if failed is None else np.ascontiguousarray(failed, dtype=np.uint8)
    assert fl is None or fl.shape == (B,)
    pf = None if prefill is None else np.array([prefill], dtype=np.uint64)
    L.check(L.lib().mof_dd_test_gather(dd._h, B, L.ptr(src), None if fl is None else L.ptr(fl),
                                       None if pf is None else L.ptr(pf), L.ptr(V)))
    return V


def dd_pcg_inner(dd: "DecomposedMesh", parts, rhs, rtol, cap, precond="jacobi", precision="mixed", sentinel=None,
                 a_system=-1) -> dict:
    """Tests only (mof_dd_test_pcg_inner): the production decomposed inner PCG
    of the handle's last batch on ``rhs`` (one (B, n_loc, 2) float64 array per
    part, local order), capped at ``cap`` iterations. Returns ``parts``: per
    part a dict in the format of :func:`mofhip.mesh.pcg_inner` (``x, r, z, p,
    q, words, z_words, sys, dinv, A`` and the shared ``scal``), plus the shared
    ``scal`` (2 slots, B, 3), ``part_rzrr`` (2, P, B, nmax, 2), ``part_pq`` (2, P, B,
    nmax), ``nmax, iterations, slowest``."""
    from .mesh import SYS_STRIDE, _sys_rows
    B = rhs[0].shape[0]
    assert all(v.shape == (B, p.N, 2) for v, p in zip(rhs, parts))
    amg = {"jacobi": 0, "amg": 1}[precond]
    dt = {"mixed": np.float32, "f64": np.float64}[precision]
    wt = {"mixed": np.uint32, "f64": np.uint64}[precision]
    src = _cat(rhs, np.float64)
    nloc = sum(p.N for p in parts)
    nbs = [int(p.info()["sell_blocks"]) for p in parts]
    vec = {k: np.zeros(B * nloc * 2, dtype=wt) for k in "xrzpq"}
    si = np.zeros((len(parts), B, SYS_STRIDE), dtype=np.int32)
    sd = np.zeros((len(parts), B, SYS_STRIDE), dtype=np.float64)
    dinv = np.zeros(B * nloc * 4, dtype=dt)
    A = np.zeros(sum(nbs) * 4, dtype=dt)
    meta = np.zeros(6, dtype=np.int32)
    P = parts[0].nparts
    nmax = PartHandle(dd, 0).nmax  # as the last solve left it
    rzrr = np.zeros((2, P, B, nmax, 2))
    pq = np.zeros((2, P, B, nmax))
    scal = np.zeros((2, B, 3))
    sw = None if sentinel is None else np.array([sentinel], dtype=np.uint32)
    L.check(L.lib().mof_dd_test_pcg_inner(
        dd._h, B, L.ptr(src), float(rtol), amg, {"mixed": L.MOF_PREC_MIXED, "f64": L.MOF_PREC_F64}[precision], int(cap),
        None if sw is None else L.ptr(sw), L.ptr(vec["x"]), L.ptr(vec["r"]), L.ptr(vec["z"]), L.ptr(vec["p"]),
        L.ptr(vec["q"]), L.ptr(si), L.ptr(sd), L.ptr(dinv), int(a_system), L.ptr(A), L.ptr(rzrr), L.ptr(pq),
        L.ptr(scal), L.ptr(meta)))
    assert meta[0] == nmax and meta[1] == P and meta[4] == SYS_STRIDE and meta[5] == len(parts), meta
    sp = {k: _split(vec[k], parts, B) for k in "xrzpq"}
    dv = _split(dinv, parts, B, 4)
    out = {"parts": [], "scal": scal, "part_rzrr": rzrr, "part_pq": pq, "nmax": nmax, "iterations": int(meta[2]),
           "slowest": int(meta[3])}
    q = 0
    for l, p in enumerate(parts):
        o = {k: sp[k][l].view(dt) for k in "xrzpq"}
        o["words"] = {k: sp[k][l] for k in "xrzpq"}
        o["z_words"] = sp["z"][l]
        o.update(scal=scal, sys=_sys_rows(si[l], sd[l]), dinv=None if amg else dv[l].reshape(B, p.N, 2, 2),
                 A=A[q:q + 4 * nbs[l]].reshape(nbs[l], 2, 2).copy() if a_system >= 0 else None)
        q += 4 * nbs[l]
        out["parts"].append(o)
    return out
