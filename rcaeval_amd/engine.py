"""Device engine: thin Python owner of one ``pcg_handle`` per GPU.

PyTorch-ROCm is used only as plumbing — device buffers (``tensor.data_ptr()``), the
stream the handle runs on, and (in ``rcaeval_amd.dist``) ``torch.distributed``. All
arithmetic runs in the HIP kernels of ``libpcgpu.so``.
"""
from __future__ import annotations

import contextlib
import ctypes
import time

import numpy as np

from . import _lib
from ._lib import PcgRecord, PcgScalerCase, PcgStats, check

_ENGINES: dict = {}

RECORD_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("d", np.int32),
                         ("s", np.int32, _lib.PCG_MAX_DEPTH), ("p", np.float64)], align=True)
assert RECORD_DTYPE.itemsize == ctypes.sizeof(PcgRecord)


def _torch():
    import torch
    return torch


class SkeletonOut:
    """Result of one device skeleton run.

    The skeleton stays resident in HBM (``removed_level_dev``, ``sep_xy_dev``,
    ``sep_bits_dev`` torch tensors); the numpy views (``removed_level``, ``sep_xy``,
    ``sep_bits``) are copied to the host on first access.
    """

    rc = 0      # PCG_OK, or a batch case's own error code (Engine.skeleton_batch raises nothing per case)

    def __init__(self, n, rl_dev, xy_dev, bits_dev, deg_levels, stats, records=None, near_alpha=None,
                 device_ms=0.0):
        self.n = n
        self.removed_level_dev = rl_dev
        self.sep_xy_dev = xy_dev
        self.sep_bits_dev = bits_dev
        self.deg_levels = deg_levels          # levels x n int32 (host)
        self.stats = stats
        self.records = records                # RECORD_DTYPE (PCG_FLAG_RECORD)
        self.near_alpha = near_alpha
        self.device_ms = device_ms
        self.extra: dict = {}
        self._host: dict = {}

    def _h(self, key, t):
        if key not in self._host:
            self._host[key] = t.cpu().numpy()
        return self._host[key]

    @property
    def removed_level(self) -> np.ndarray:      # n x n int8, -1 = edge survives
        return self._h("rl", self.removed_level_dev)

    @property
    def sep_xy(self) -> np.ndarray:             # R x 2 int32, ordered removed pairs, non-empty union
        return self._h("xy", self.sep_xy_dev)

    @property
    def sep_bits(self) -> np.ndarray:           # R x W uint64, x-side union (global node bits)
        return self._h("bits", self.sep_bits_dev).view(np.uint64)

    @property
    def levels(self) -> int:
        return int(self.stats["levels"])

    @property
    def adj(self) -> np.ndarray:
        a = self.removed_level == -1
        np.fill_diagonal(a, False)
        return a


class Engine:
    """One handle on one HIP device."""

    def __init__(self, device: int = 0, stream=None):
        """``stream``: the torch stream the handle runs on (default: the current stream of
        ``device`` in the calling thread)."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.EngineUnavailable("no HIP device is visible (torch.cuda.is_available() is False)")
        self.lib = _lib.load()
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        h = ctypes.c_void_p()
        rc = self.lib.pcg_create(self.device_index, ctypes.byref(h))
        if rc != 0:
            raise _lib.PcgError(rc, f"pcg_create(device={device}) failed")
        self.h = h
        if stream is None:
            with torch.cuda.device(self.device):
                stream = torch.cuda.current_stream(self.device)
        self.stream = stream
        check(self.h, self.lib.pcg_set_stream(self.h, ctypes.c_void_p(stream.cuda_stream)), "pcg_set_stream")
        # sepset rows exported straight into engine-owned buffers (pcg_set_sepset_buffers): the
        # buffer (W, capacity, xy, bits) armed for the current call, and the row bound per n
        self._sep_buf = None
        self._sep_armed = None
        self._sep_need: dict = {}

    def close(self):
        if getattr(self, "h", None):
            self.lib.pcg_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ tuning knobs
    def get_tuning(self, key: str) -> int:
        v = ctypes.c_int64()
        check(self.h, self.lib.pcg_get_tuning(self.h, _lib.TUNE_KEYS[key], ctypes.byref(v)), "pcg_get_tuning")
        return v.value

    def set_tuning(self, key: str, value: int) -> None:
        check(self.h, self.lib.pcg_set_tuning(self.h, _lib.TUNE_KEYS[key], int(value)), f"pcg_set_tuning({key})")

    @contextlib.contextmanager
    def tuned(self, **knobs):
        """Set pcg_set_tuning knobs (``eng.tuned(SMALL=0, LDS_DEEP=12)``) for the ``with`` body,
        restoring the previous values after it."""
        old = {k: self.get_tuning(k) for k in knobs}
        try:
            for k, v in knobs.items():
                self.set_tuning(k, v)
            yield self
        finally:
            for k, v in old.items():
                self.set_tuning(k, v)

    def image_totals(self, depth: int) -> tuple:
        """(host, device) size in doubles of ``depth``'s node images in the last level-loop run, when
        they were built behind the previous depth's barrier from the device's own scan; (-1, -1)
        when they were not (pcg_level_image_totals)."""
        hd, dd = ctypes.c_int64(), ctypes.c_int64()
        check(self.h, self.lib.pcg_level_image_totals(self.h, int(depth), ctypes.byref(hd), ctypes.byref(dd)),
              "pcg_level_image_totals")
        return hd.value, dd.value

    def k1_plan_signature(self, n: int, N: int) -> int:
        v = ctypes.c_int64()
        check(self.h, self.lib.pcg_k1_plan_signature(self.h, int(n), int(N), ctypes.byref(v)), "pcg_k1_plan_signature")
        return v.value

    def k1_crt_plan(self, n: int, N: int) -> dict:
        """The split-K plan a one-rank ``corr`` of (n, N) runs under this engine's knobs
        (pcg_k1_crt_plan); every value 0 when (n, N) does not take the CRT path."""
        v = (ctypes.c_int64 * 8)()
        check(self.h, self.lib.pcg_k1_crt_plan(self.h, int(n), int(N), v), "pcg_k1_crt_plan")
        return dict(zip(("tiles", "moduli", "tA", "ksA", "kbA", "ksB", "kbB", "units"), (int(x) for x in v)))

    # ------------------------------------------------------------------ helpers
    def to_device(self, a) -> "object":
        torch = _torch()
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=torch.float64).contiguous()
        arr = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        return torch.from_numpy(arr).to(self.device)

    def _strided(self, a):
        """True for an fp64 2-d tensor already on this device whose rows are contiguous
        (``stride(1) == 1``, ``stride(0) >= ncols``): the ABI takes it in place with its row
        stride as the leading dimension."""
        torch = _torch()
        return (isinstance(a, torch.Tensor) and a.device == self.device and a.dtype == torch.float64
                and a.dim() == 2 and a.shape[1] >= 1 and a.stride(1) == 1 and a.stride(0) >= a.shape[1])

    def _ld(self, a):
        """(device tensor, leading dimension) of a 2-d input: a row-strided device view is used in
        place (``_strided``), host arrays and every other tensor are uploaded / made contiguous."""
        if not self._strided(a):
            a = self.to_device(a)
        if a.dim() != 2:
            raise ValueError("expected a 2-d array")
        return a, (int(a.stride(0)) if a.shape[0] > 1 else int(a.shape[1]))

    def _out_view(self, out, n: int):
        """(n x n fp64 device tensor, ldc) for a correlation result: a fresh contiguous tensor, or
        the caller's row-strided device view ``out`` written in place (its padding untouched)."""
        torch = _torch()
        if out is None:
            return torch.empty((n, n), dtype=torch.float64, device=self.device), n
        if not self._strided(out) or tuple(out.shape) != (n, n):
            raise ValueError(f"out= must be a {n} x {n} float64 view on {self.device} with contiguous rows")
        return out, (int(out.stride(0)) if n > 1 else n)

    def sync(self):
        _torch().cuda.synchronize(self.device)

    # ------------------------------------------------------------------ K1
    def corr(self, X, out=None) -> "object":
        """``np.corrcoef(X.T)`` of an N x n array on the GPU; returns an n x n fp64 tensor.
        A row-strided fp64 device view of X is read in place (``ldx`` = its row stride);
        ``out``: an n x n device view to write C into (``ldc`` = its row stride), returned."""
        Xd, ldx = self._ld(X)
        N, n = Xd.shape
        C, ldc = self._out_view(out, n)
        check(self.h, self.lib.pcg_corr(self.h, ctypes.c_void_p(Xd.data_ptr()), N, n, ldx,
                                        ctypes.c_void_p(C.data_ptr()), ldc), "pcg_corr")
        return C

    def corr_shard(self, X, rank: int, world: int):
        """This rank's share of the sharded K1 (see ``pcg_corr_shard``), a flat fp64 tensor."""
        torch = _torch()
        Xd = self.to_device(X)
        N, n = Xd.shape
        nbytes = ctypes.c_int64()
        check(self.h, self.lib.pcg_corr_shard_bytes(self.h, n, N, int(world), ctypes.byref(nbytes)),
              "pcg_corr_shard_bytes")
        packed = torch.empty(nbytes.value // 8, dtype=torch.float64, device=self.device)
        check(self.h, self.lib.pcg_corr_shard(self.h, ctypes.c_void_p(Xd.data_ptr()), N, n, n, int(rank),
                                              int(world), ctypes.c_void_p(packed.data_ptr())), "pcg_corr_shard")
        return packed

    def corr_shard_finish(self, gathered, N: int, n: int, world: int):
        """C from the rank-major concatenation of every rank's share (same handle as ``corr_shard``)."""
        torch = _torch()
        g = gathered.contiguous()
        C = torch.empty((n, n), dtype=torch.float64, device=self.device)
        check(self.h, self.lib.pcg_corr_shard_finish(self.h, ctypes.c_void_p(g.data_ptr()), int(N), int(n),
                                                     int(world), ctypes.c_void_p(C.data_ptr()), n),
              "pcg_corr_shard_finish")
        return C

    # ------------------------------------------------------------------ native multi-GPU
    def comm_unique_id(self) -> bytes:
        """RCCL unique id (PCG_COMM_ID_BYTES) for pcg_comm_init; rank 0 makes it."""
        buf = ctypes.create_string_buffer(128)
        check(self.h, self.lib.pcg_comm_unique_id(buf, 128), "pcg_comm_unique_id")
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int) -> None:
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        check(self.h, self.lib.pcg_comm_init(self.h, buf, int(rank), int(world)), "pcg_comm_init")

    def comm_init_group(self, group, rank: int) -> None:
        """Attach this handle as ``rank`` of an in-process ``rcaeval_amd.dist.LocalGroup``
        (pcg_comm_init_group): the native driver's collectives then run host-staged between the
        group's handles, which other threads of this process drive."""
        check(self.h, self.lib.pcg_comm_init_group(self.h, group.g, int(rank)), "pcg_comm_init_group")

    def comm_destroy(self) -> None:
        check(self.h, self.lib.pcg_comm_destroy(self.h), "pcg_comm_destroy")

    def corr_sharded(self, X):
        """K1 on the handle's communicator (pcg_corr_sharded): bitwise ``corr``."""
        torch = _torch()
        Xd = self.to_device(X)
        N, n = Xd.shape
        C = torch.empty((n, n), dtype=torch.float64, device=self.device)
        check(self.h, self.lib.pcg_corr_sharded(self.h, ctypes.c_void_p(Xd.data_ptr()), N, n, n,
                                                ctypes.c_void_p(C.data_ptr()), n), "pcg_corr_sharded")
        return C

    def skeleton_sharded(self, C, N: int, alpha: float = 0.05, max_depth: int = -1, flags: int = 0) -> SkeletonOut:
        """The edge-sharded skeleton with the level loop in C (pcg_skeleton_sharded)."""
        torch = _torch()
        Cd = self.to_device(C)
        n = Cd.shape[0]
        rl = torch.empty((n, n), dtype=torch.int8, device=self.device)
        st = PcgStats()
        rc = self.lib.pcg_skeleton_sharded(self.h, ctypes.c_void_p(Cd.data_ptr()), n, n, int(N), float(alpha),
                                           int(max_depth), int(flags), ctypes.c_void_p(rl.data_ptr()),
                                           ctypes.byref(st))
        check(self.h, rc, "pcg_skeleton_sharded")
        # (results are stream-ordered on the handle's stream: no host sync here)
        return self._collect(n, rl, st, None)

    # ------------------------------------------------------------------ K2/K3
    def _sep_arm(self, n: int) -> None:
        """Let the next one-GPU run export its sepset rows straight into an engine-owned buffer
        (pcg_set_sepset_buffers), sized from the last run's row bound for this n: the result then
        holds views of it and no copy follows the call. A buffer that any live tensor still views
        (an earlier result, or a slice a caller kept) is never written again: a fresh one is
        allocated and the old one stays with its viewers."""
        import sys
        need = self._sep_need.get(n, 0)
        self._sep_armed = None
        if need <= 0:          # first run of this n: the handle's own buffers, then a copy
            return
        torch = _torch()
        W = (n + 63) // 64
        buf = self._sep_buf
        # (2 references: self._sep_buf's tuple and getrefcount's argument; a live view adds one)
        if buf is None or buf[0] != W or buf[1] < need or sys.getrefcount(buf[2]) > 2 or sys.getrefcount(buf[3]) > 2:
            cap = need + need // 4 + 64
            buf = (W, cap, torch.empty((cap, 2), dtype=torch.int32, device=self.device),
                   torch.empty((cap, W), dtype=torch.int64, device=self.device))
            self._sep_buf = buf
        check(self.h, self.lib.pcg_set_sepset_buffers(self.h, ctypes.c_void_p(buf[2].data_ptr()),
                                                      ctypes.c_void_p(buf[3].data_ptr()), buf[1]),
              "pcg_set_sepset_buffers")
        self._sep_armed = buf

    def _sep_disarm(self) -> None:
        if self._sep_armed is not None:
            self.lib.pcg_set_sepset_buffers(self.h, None, None, 0)

    def _banned(self, banned, n: int):
        """Device copy of the n x n uint8 banned-pair mask, registered with the handle (or None)."""
        if banned is None:
            return None
        b = np.ascontiguousarray(banned, dtype=np.uint8)
        if b.shape != (n, n):
            raise ValueError(f"banned mask shape {b.shape} != ({n}, {n})")
        bd = _torch().from_numpy(b).to(self.device)          # bytes, not to_device's float64
        check(self.h, self.lib.pcg_set_forbidden_pairs(self.h, ctypes.c_void_p(bd.data_ptr())),
              "pcg_set_forbidden_pairs")
        return bd

    def _events(self):
        """The call's (start, end) timing events, created once per engine (a fresh pair per call
        costs two event creations on the host path between steps)."""
        if getattr(self, "_ev_pair", None) is None:
            torch = _torch()
            self._ev_pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        return self._ev_pair

    def _unban(self, bd) -> None:
        if bd is not None:
            self.lib.pcg_set_forbidden_pairs(self.h, None)

    def skeleton(self, C, N: int, alpha: float = 0.05, max_depth: int = -1, flags: int = 0,
                 record_capacity: int = 0, record_sample: tuple = (0, 0), banned=None) -> SkeletonOut:
        """``record_sample=(modulus, residue)``: with PCG_FLAG_RECORD keep only the tests of the
        canonical pairs (a, b) with (a*n + b) % modulus == residue (full-size parity samples).
        ``banned``: n x n mask of pairs removed at the end of depth 0 (background knowledge,
        ``rcaeval_amd.background.banned_pairs``)."""
        torch = _torch()
        Cd, ldc = self._ld(C)
        n = Cd.shape[0]
        rl = torch.empty((n, n), dtype=torch.int8, device=self.device)
        if record_capacity:
            check(self.h, self.lib.pcg_set_capacity(self.h, int(record_capacity), 0), "pcg_set_capacity")
        check(self.h, self.lib.pcg_set_record_sample(self.h, int(record_sample[0]), int(record_sample[1])),
              "pcg_set_record_sample")
        st = PcgStats()
        ev0, ev1 = self._events()
        bd = self._banned(banned, n)
        self._sep_arm(n)
        try:
            ev0.record()
            rc = self.lib.pcg_skeleton(self.h, ctypes.c_void_p(Cd.data_ptr()), n, ldc, int(N), float(alpha),
                                       int(max_depth), int(flags), ctypes.c_void_p(rl.data_ptr()),
                                       ctypes.byref(st))
            ev1.record()
        finally:
            self._unban(bd)
            self._sep_disarm()
        check(self.h, rc, "pcg_skeleton")
        t0 = time.perf_counter()
        out = self._collect(n, rl, st, (ev0, ev1))
        out.extra["collect_ms"] = 1000.0 * (time.perf_counter() - t0)
        out.extra["device_ms"] = out.device_ms
        return out

    def corr_skeleton(self, X, alpha: float = 0.05, max_depth: int = -1, flags: int = 0, record_capacity: int = 0,
                      banned=None, out=None):
        """K1 + stable skeleton in one C call (``pcg_pc_skeleton``); returns (SkeletonOut, C).
        X and ``out`` as in ``corr``."""
        torch = _torch()
        Xd, ldx = self._ld(X)
        N, n = Xd.shape
        C, ldc = self._out_view(out, n)
        rl = torch.empty((n, n), dtype=torch.int8, device=self.device)
        if record_capacity:
            check(self.h, self.lib.pcg_set_capacity(self.h, int(record_capacity), 0), "pcg_set_capacity")
        check(self.h, self.lib.pcg_set_record_sample(self.h, 0, 0), "pcg_set_record_sample")
        st = PcgStats()
        ev0, ev1 = self._events()
        bd = self._banned(banned, n)
        self._sep_arm(n)
        try:
            ev0.record()
            rc = self.lib.pcg_pc_skeleton(self.h, ctypes.c_void_p(Xd.data_ptr()), N, n, ldx,
                                          ctypes.c_void_p(C.data_ptr()), ldc, float(alpha), int(max_depth), int(flags),
                                          ctypes.c_void_p(rl.data_ptr()), ctypes.byref(st))
            ev1.record()
        finally:
            self._unban(bd)
            self._sep_disarm()
        check(self.h, rc, "pcg_pc_skeleton")
        t0 = time.perf_counter()
        out = self._collect(n, rl, st, (ev0, ev1))
        out.extra["collect_ms"] = 1000.0 * (time.perf_counter() - t0)
        out.extra["device_ms"] = out.device_ms
        return out, C

    def skeleton_batch(self, Cs_or_Xs, Ns=None, alpha: float = 0.05, max_depth: int = -1, flags: int = 0,
                       from_data: bool = False) -> list:
        """Many small cases (2 <= n <= 64) in one launch and one host wait (``pcg_skeleton_batch``).

        ``Cs_or_Xs``: one n x n correlation matrix per case with its sample count in ``Ns``, or —
        ``from_data=True`` — one N x n data array per case (``Ns`` is then taken from the arrays;
        the batched K1 computes each C, kept as ``out.extra["C"]``). The cases are packed into one
        device allocation each for X / C, removal depths, sepset (x, y) and sepset words; every
        result holds views of its own slice, already copied to the host in one transfer each.
        A case that failed (singular / math domain) raises nothing: its ``SkeletonOut.rc`` and
        ``stats["error"]`` carry the code. ``flags``: PCG_FLAG_FULL_P and PCG_FLAG_EXACT_ALL."""
        torch = _torch()
        arrs = [a if isinstance(a, torch.Tensor) else np.ascontiguousarray(np.asarray(a, dtype=np.float64))
                for a in Cs_or_Xs]
        B = len(arrs)
        if B == 0:
            return []
        for a in arrs:
            if a.ndim != 2 or (not from_data and a.shape[0] != a.shape[1]):
                raise ValueError(f"skeleton_batch: case of shape {tuple(a.shape)}")
        ns = [int(a.shape[1]) for a in arrs]
        if from_data:
            Nl = [int(a.shape[0]) for a in arrs]
        else:
            if Ns is None:
                raise ValueError("skeleton_batch: Ns (one sample count per case) is required for correlation input")
            Nl = [int(Ns)] * B if np.isscalar(Ns) else [int(v) for v in Ns]
            if len(Nl) != B:
                raise ValueError("skeleton_batch: one N per case")
        # one packed device buffer per kind — unless every case is a row-strided device view
        # (_strided): the cases then point at the views with their own leading dimensions
        views = all(self._strided(a) for a in arrs)
        if views:
            flat = None
        elif all(isinstance(a, np.ndarray) for a in arrs):
            # packed in a page-locked staging buffer kept by the engine (grow-only), one H2D copy;
            # the copy is blocking, so the buffer is free again when the next batch packs into it
            total = sum(a.size for a in arrs)
            pin = getattr(self, "_batch_pin", None)
            if pin is None or pin.numel() < total:
                pin = self._batch_pin = torch.empty(total + total // 4, dtype=torch.float64, pin_memory=True)
            stage, o = pin.numpy(), 0
            for a in arrs:
                stage[o:o + a.size] = a.reshape(-1)
                o += a.size
            flat = torch.empty(total, dtype=torch.float64, device=self.device)
            flat.copy_(pin[:total])
        else:
            flat = torch.cat([self.to_device(a).reshape(-1) for a in arrs])
        sq = np.array([n * n for n in ns], np.int64)
        rows_cap = np.array([max(n * (n - 1), 1) for n in ns], np.int64)
        in_off = np.concatenate([[0], np.cumsum([a.shape[0] * a.shape[1] for a in arrs])])
        sq_off = np.concatenate([[0], np.cumsum(sq)])
        row_off = np.concatenate([[0], np.cumsum(rows_cap)])
        # (from_data: the batched K1's C stays packed, also for views)
        Call = torch.empty(int(sq_off[-1]), dtype=torch.float64, device=self.device) if from_data else flat
        rl = torch.empty(int(sq_off[-1]), dtype=torch.int8, device=self.device)
        xy = torch.empty((int(row_off[-1]), 2), dtype=torch.int32, device=self.device)
        bits = torch.empty((int(row_off[-1]), 1), dtype=torch.int64, device=self.device)
        cases = (_lib.PcgCase * B)()
        prl, pxy, pbits = rl.data_ptr(), xy.data_ptr(), bits.data_ptr()
        pin = None if views else flat.data_ptr()
        pC = None if Call is None else Call.data_ptr()
        for i in range(B):
            c = cases[i]
            c.N, c.n = Nl[i], ns[i]
            if views:
                ld = int(arrs[i].stride(0)) if arrs[i].shape[0] > 1 else ns[i]
                c.X, c.ldx = (arrs[i].data_ptr(), ld) if from_data else (None, ns[i])
                c.C, c.ldc = (pC + 8 * int(sq_off[i]), ns[i]) if from_data else (arrs[i].data_ptr(), ld)
            else:
                c.X = pin + 8 * int(in_off[i]) if from_data else None
                c.ldx = ns[i]
                c.C = pC + 8 * int(sq_off[i])
                c.ldc = ns[i]
            c.removed_level = prl + int(sq_off[i])
            c.sep_xy = pxy + 8 * int(row_off[i])
            c.sep_bits = pbits + 8 * int(row_off[i])
        res = (_lib.PcgCaseResult * B)()
        check(self.h, self.lib.pcg_skeleton_batch(self.h, cases, B, float(alpha), int(max_depth), int(flags), res),
              "pcg_skeleton_batch")
        # the call returned after the handle's stream was synchronised: every result is complete
        rl_h, xy_h, bits_h = rl.cpu().numpy(), xy.cpu().numpy(), bits.cpu().numpy()
        outs = []
        for i in range(B):
            r, n = res[i], ns[i]
            rows = int(r.sep_rows)
            s0, r0 = int(sq_off[i]), int(row_off[i])
            L = int(r.stats.levels)
            deg = np.ctypeslib.as_array(r.deg)[:L, :n].copy()
            near = np.zeros(int(r.near_alpha_count), RECORD_DTYPE)
            if len(near):
                check(self.h, self.lib.pcg_batch_near_export(self.h, i, near.ctypes.data_as(ctypes.c_void_p), len(near)),
                      "pcg_batch_near_export")
            out = SkeletonOut(n, rl[s0:s0 + n * n].view(n, n), xy[r0:r0 + rows], bits[r0:r0 + rows], deg,
                              r.stats.as_dict(), np.zeros(0, RECORD_DTYPE), near)
            out.rc = int(r.rc)
            out._host = {"rl": rl_h[s0:s0 + n * n].reshape(n, n), "xy": xy_h[r0:r0 + rows],
                         "bits": bits_h[r0:r0 + rows]}
            out.extra["C"] = arrs[i] if Call is None else Call[s0:s0 + n * n].view(n, n)
            outs.append(out)
        return outs

    def _collect(self, n: int, rl, st: PcgStats, events=None) -> SkeletonOut:
        # the sepset rows' device copies are enqueued first (they are the step's last device work);
        # the host-side results are gathered while they run
        torch = _torch()
        cnt, W = ctypes.c_int64(), ctypes.c_int32()
        check(self.h, self.lib.pcg_sepset_count(self.h, ctypes.byref(cnt), ctypes.byref(W)), "pcg_sepset_count")
        tgt, need = ctypes.c_int32(), ctypes.c_int64()
        check(self.h, self.lib.pcg_sepset_target(self.h, ctypes.byref(tgt), ctypes.byref(need)), "pcg_sepset_target")
        if need.value > 0:
            self._sep_need[n] = int(need.value)
        buf, self._sep_armed = self._sep_armed, None
        if tgt.value and buf is not None and buf[0] == W.value:
            xy, bits = buf[2][:cnt.value], buf[3][:cnt.value]      # rows already in place: views
        else:
            xy = torch.empty((cnt.value, 2), dtype=torch.int32, device=self.device)
            bits = torch.empty((cnt.value, W.value), dtype=torch.int64, device=self.device)
            if cnt.value:
                check(self.h, self.lib.pcg_sepset_export_device(self.h, ctypes.c_void_p(xy.data_ptr()),
                                                                ctypes.c_void_p(bits.data_ptr()), cnt.value),
                      "pcg_sepset_export_device")
        L = st.levels
        deg = np.zeros((max(L, 1), n), np.int32)
        if L:
            check(self.h, self.lib.pcg_degrees(self.h, deg.ctypes.data_as(ctypes.c_void_p), deg.size),
                  "pcg_degrees")
        rc_, nc_ = ctypes.c_int64(), ctypes.c_int64()
        check(self.h, self.lib.pcg_record_count(self.h, ctypes.byref(rc_), ctypes.byref(nc_)), "pcg_record_count")
        rec = np.zeros(rc_.value, RECORD_DTYPE)
        near = np.zeros(nc_.value, RECORD_DTYPE)
        if rc_.value or nc_.value:
            check(self.h, self.lib.pcg_record_export(self.h, rec.ctypes.data_as(ctypes.c_void_p), rc_.value,
                                                     near.ctypes.data_as(ctypes.c_void_p), nc_.value),
                  "pcg_record_export")
        # the sepset rows were copied on the handle's stream: a caller on that stream is ordered
        # after them; any other current stream waits for them
        if torch.cuda.current_stream(self.device) != self.stream:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
        device_ms = 0.0
        if events is not None:      # (start, end) events around the call
            events[1].synchronize()     # the call returned after its last device phase; the end event follows it
            device_ms = events[0].elapsed_time(events[1])
        return SkeletonOut(n, rl, xy, bits, deg[:L].copy(), st.as_dict(), rec, near, device_ms)

    # ------------------------------------------------------------------ batched CI tests
    def fisherz_batch(self, C, N: int, rows: np.ndarray):
        """Fisher-z p of canonical rows ``[a, b, d, s_0..s_{d-1}, pad]`` (int32, count x stride)
        on the device correlation ``C``; returns (p float64, status int32) host arrays."""
        torch = _torch()
        Cd, ldc = self._ld(C)
        n = Cd.shape[0]
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        count, stride = rows.shape
        t = torch.from_numpy(rows).to(self.device)
        p = torch.empty(count, dtype=torch.float64, device=self.device)
        st = torch.empty(count, dtype=torch.int32, device=self.device)
        check(self.h, self.lib.pcg_fisherz_batch(self.h, ctypes.c_void_p(Cd.data_ptr()), n, ldc, int(N),
                                                 ctypes.c_void_p(t.data_ptr()), int(stride), int(count),
                                                 ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(st.data_ptr())),
              "pcg_fisherz_batch")
        return p.cpu().numpy(), st.cpu().numpy()

    def chisq_batch(self, data_dev, card_dev, N: int, n: int, rows: np.ndarray, g_sq: bool, max_cells: int):
        """Contingency statistics of canonical rows ``[a, b, d, s..]`` (``pcg_chisq_batch``) on
        variable-major int32 codes ``data_dev`` (n x N); returns (stat, df, status) host arrays."""
        torch = _torch()
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        count, stride = rows.shape
        t = torch.from_numpy(rows).to(self.device)
        stat = torch.empty(count, dtype=torch.float64, device=self.device)
        df = torch.empty(count, dtype=torch.int64, device=self.device)
        st = torch.empty(count, dtype=torch.int32, device=self.device)
        check(self.h, self.lib.pcg_chisq_batch(self.h, ctypes.c_void_p(data_dev.data_ptr()), int(N), int(n),
                                               ctypes.c_void_p(card_dev.data_ptr()), ctypes.c_void_p(t.data_ptr()),
                                               int(stride), int(count), int(bool(g_sq)), int(max_cells),
                                               ctypes.c_void_p(stat.data_ptr()), ctypes.c_void_p(df.data_ptr()),
                                               ctypes.c_void_p(st.data_ptr())), "pcg_chisq_batch")
        return stat.cpu().numpy(), df.cpu().numpy(), st.cpu().numpy()

    def granger(self, X, maxlag: int = 3) -> dict:
        """Pairwise Granger regressions of a T x n array (``pcg_granger``): host arrays ``ssr_r``,
        ``ssr_u``, ``tss`` (float64), ``rank``, ``status`` (int32), each n x n x maxlag with item
        [i, j, L - 1] = column j causing column i at lag L, and ``exact_items``, the number of
        items the exact path computed. ``T <= 3 * maxlag + 1`` raises ``ValueError``."""
        torch = _torch()
        Xd, ldx = self._ld(X)
        T, n = Xd.shape
        shape = (n, n, int(maxlag))
        f = [torch.empty(shape, dtype=torch.float64, device=self.device) for _ in range(3)]
        k = [torch.empty(shape, dtype=torch.int32, device=self.device) for _ in range(2)]
        exact = ctypes.c_int64()
        check(self.h, self.lib.pcg_granger(self.h, ctypes.c_void_p(Xd.data_ptr()), int(T), int(n), ldx, int(maxlag),
                                           *(ctypes.c_void_p(t.data_ptr()) for t in f + k), ctypes.byref(exact)),
              "pcg_granger")
        out = {name: t.cpu().numpy() for name, t in zip(("ssr_r", "ssr_u", "tss", "rank", "status"), f + k)}
        out["exact_items"] = int(exact.value)
        return out

    # ------------------------------------------------------------------ cMLP
    def _rows_f32(self, X):
        """(device tensor, T, p, ldx) of a T x p input for the fp32 cMLP kernels: an fp32 tensor
        already on this device whose rows are contiguous is used in place with its row stride,
        anything else is cast (float64 -> float32, as the reference does) and uploaded."""
        torch = _torch()
        if not (isinstance(X, torch.Tensor) and X.device == self.device and X.dtype == torch.float32 and X.dim() == 2
                and X.shape[1] >= 1 and X.stride(1) == 1 and X.stride(0) >= X.shape[1]):
            if isinstance(X, torch.Tensor):
                X = X.to(device=self.device, dtype=torch.float32).contiguous()
            else:
                X = torch.from_numpy(np.array(X, dtype=np.float32, order="C")).to(self.device)
        if X.dim() != 2:
            raise ValueError("expected a T x p array")
        return X, int(X.shape[0]), int(X.shape[1]), int(X.stride(0)) if X.shape[0] > 1 else int(X.shape[1])

    def _cmlp_params(self, params, p: int, lag: int, hidden: int):
        """A private flat fp32 device copy of the packed parameters (the kernels update it in place)."""
        torch = _torch()
        if isinstance(params, torch.Tensor):
            P = params.detach().to(device=self.device, dtype=torch.float32).reshape(-1).clone()
        else:
            P = torch.from_numpy(np.array(params, dtype=np.float32).reshape(-1)).to(self.device)
        want = p * (hidden * p * lag + 2 * hidden + 1)
        if P.numel() != want:
            raise ValueError(f"cmlp: packed parameters hold {P.numel()} floats, p={p} lag={lag} hidden={hidden} needs {want}")
        return P

    def cmlp_limits(self) -> dict:
        """The limits of the cMLP kernels (``pcg_cmlp_limits``)."""
        from .graph_construction.cmlp import limits
        return limits()

    def cmlp_steps(self, X, params, k: int, lag: int = 5, hidden: int = 100, lr: float = 5e-2, lam: float = 0.002,
                   lam_ridge: float = 1e-2) -> tuple:
        """``k`` ISTA iterations of the cMLP on a T x p array with no checks (``pcg_cmlp_steps``).
        ``params``: the packed parameters (``graph_construction.cmlp.pack``), host or device; a copy
        is updated. Returns (packed fp32 device tensor, host float64 array of the p per-network
        MSEs after the last step). ``T <= lag`` raises ``ValueError``."""
        Xd, T, p, ldx = self._rows_f32(X)
        P = self._cmlp_params(params, p, int(lag), int(hidden))
        smooth = np.empty(p, dtype=np.float64)
        check(self.h, self.lib.pcg_cmlp_steps(self.h, ctypes.c_void_p(Xd.data_ptr()), T, p, ldx, int(lag), int(hidden),
                                              ctypes.c_void_p(P.data_ptr()), float(lr), float(lam), float(lam_ridge),
                                              int(k), smooth.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
              "pcg_cmlp_steps")
        return P, smooth

    def cmlp_train(self, X, params, max_iter: int, lag: int = 5, hidden: int = 100, lr: float = 5e-2,
                   lam: float = 0.002, lam_ridge: float = 1e-2, check_every: int = 1000, lookback: int = 5) -> dict:
        """The cMLP's ISTA training loop with its early-stopping checks (``pcg_cmlp_train``) on a
        T x p array. Returns ``params`` (packed fp32 device tensor: the best check's snapshot),
        ``losses`` (host float64, one mean loss per check), ``n_checks``, ``best_it``, ``last_it``.
        Raises ``ValueError`` where the reference raises: ``T <= lag``, ``max_iter < check_every``,
        a first check whose loss is NaN or Inf."""
        Xd, T, p, ldx = self._rows_f32(X)
        P = self._cmlp_params(params, p, int(lag), int(hidden))
        losses = np.zeros(max(1, int(max_iter) // max(1, int(check_every))), dtype=np.float64)
        nc, bi, li = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(self.h, self.lib.pcg_cmlp_train(self.h, ctypes.c_void_p(Xd.data_ptr()), T, p, ldx, int(lag), int(hidden),
                                              ctypes.c_void_p(P.data_ptr()), float(lr), float(lam), float(lam_ridge),
                                              int(max_iter), int(check_every), int(lookback),
                                              losses.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                              ctypes.byref(nc), ctypes.byref(bi), ctypes.byref(li)),
              "pcg_cmlp_train")
        return {"params": P, "losses": losses[:nc.value].copy(), "n_checks": int(nc.value), "best_it": int(bi.value),
                "last_it": int(li.value)}

    def _rows(self, X):
        """(device tensor, T, n, ldx) of a T x n input: an fp64 tensor already on this device whose
        rows are contiguous is used in place with its row stride, anything else is uploaded."""
        if not self._strided(X):
            X = self.to_device(X)
        if X.dim() != 2:
            raise ValueError("expected a T x n array")
        return X, int(X.shape[0]), int(X.shape[1]), int(X.stride(0)) if X.shape[0] > 1 else int(X.shape[1])

    def lingam_pair_scores(self, X):
        """One DirectLiNGAM search step over all columns of a T x n array
        (``pcg_lingam_pair_scores``): host arrays ``D`` (n x n, antisymmetric, zero diagonal) and
        ``M`` (n). n outside 1..4096 or T < 2 raises ``ValueError``."""
        torch = _torch()
        Xd, T, n, ldx = self._rows(X)
        D = torch.empty((n, n), dtype=torch.float64, device=self.device)
        M = torch.empty(n, dtype=torch.float64, device=self.device)
        check(self.h, self.lib.pcg_lingam_pair_scores(self.h, ctypes.c_void_p(Xd.data_ptr()), T, n, ldx,
                                                      ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(M.data_ptr())),
              "pcg_lingam_pair_scores")
        return D.cpu().numpy(), M.cpu().numpy()

    def direct_lingam_order(self, X, scores: bool = False):
        """DirectLiNGAM's causal order of a T x n array (``pcg_direct_lingam_order``): an int32
        host array of the n column indices; with ``scores`` also the n x n array whose row s is
        step s's M by original column (-inf once ordered, 0 for the last step's lone candidate)."""
        torch = _torch()
        Xd, T, n, ldx = self._rows(X)
        order = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        S = torch.empty((n, n), dtype=torch.float64, device=self.device) if scores else None
        check(self.h, self.lib.pcg_direct_lingam_order(self.h, ctypes.c_void_p(Xd.data_ptr()), T, n, ldx,
                                                       ctypes.c_void_p(order.data_ptr()),
                                                       ctypes.c_void_p(S.data_ptr()) if scores else None),
              "pcg_direct_lingam_order")
        order = order[:n].cpu().numpy()
        return (order, S.cpu().numpy()) if scores else order

    # ------------------------------------------------------------------ PCMCI
    def pcmci_limits(self) -> dict:
        """The limits and fast-path guards of the PCMCI kernels (``pcg_pcmci_limits``)."""
        from .graph_construction.pcmci import limits
        return limits()

    def pcmci_parents(self, X, tau_max: int, pc_alpha: float, check_status: bool = True) -> dict:
        """PC1 of every target of a T x n array (``pcg_pcmci_parents``), which also leaves the
        lag-expanded correlation matrix in the handle for ``pcmci_mci``. Host results: ``parents``
        (per target the ordered list of ``(i, -lag)``), ``val_min`` (same shape), ``levels``,
        ``tests``, ``status`` (n each) and ``exact_items``; ``ids`` / ``count`` are the device
        arrays ``pcmci_mci`` takes. With ``check_status`` a status 1 (a constant window) or 2
        (non-finite input) raises ``ValueError``."""
        from .graph_construction import pcmci as pm
        torch = _torch()
        Xd, T, n, ldx = self._rows(X)
        tau_max = int(tau_max)
        lim = pm.limits()
        pcap = lim["z_cap"] + 2
        crit = np.ascontiguousarray(pm.critical_values(T - 2 * tau_max, float(pc_alpha), lim["z_cap"] + 1))
        ids = torch.zeros((max(n, 1), pcap), dtype=torch.int32, device=self.device)
        vmin = torch.zeros((max(n, 1), pcap), dtype=torch.float64, device=self.device)
        k = [torch.zeros(max(n, 1), dtype=torch.int32, device=self.device) for _ in range(3)]     # count, levels, status
        tests = torch.zeros(max(n, 1), dtype=torch.int64, device=self.device)
        exact = ctypes.c_int64()
        check(self.h, self.lib.pcg_pcmci_parents(
            self.h, ctypes.c_void_p(Xd.data_ptr()), T, n, ldx, tau_max, crit.ctypes.data_as(ctypes.c_void_p), len(crit),
            ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(vmin.data_ptr()), ctypes.c_void_p(k[0].data_ptr()), pcap,
            ctypes.c_void_p(k[1].data_ptr()), ctypes.c_void_p(tests.data_ptr()), ctypes.c_void_p(k[2].data_ptr()),
            ctypes.byref(exact)), "pcg_pcmci_parents")
        count, levels, status = (t.cpu().numpy() for t in k)
        out = {"ids": ids, "count": k[0], "pcap": pcap, "T": T, "n": n, "tau_max": tau_max, "levels": levels,
               "tests": tests.cpu().numpy(), "status": status, "exact_items": int(exact.value)}
        if check_status:
            pm.raise_on_status(status)
        ids_h, vmin_h = ids.cpu().numpy(), vmin.cpu().numpy()
        K = 2 * tau_max + 1
        out["parents"] = [[(int(q) // K, -(int(q) % K)) for q in ids_h[j, :min(count[j], pcap)]] for j in range(n)]
        out["val_min"] = [[float(v) for v in vmin_h[j, :min(count[j], pcap)]] for j in range(n)]
        return out

    def pcmci_mci(self, T: int, n: int, tau_max: int, parents) -> dict:
        """MCI on the correlation matrix the last ``pcmci_parents`` of the same (T, n, tau_max)
        left in the handle (``pcg_pcmci_mci``). ``parents``: that call's result, or a list of n lists
        of ``(i, -lag)``. Host arrays ``val``, ``dim`` (|Z|, -1 untested), ``status``, each
        n x n x (tau_max + 1) indexed [i, j, tau], and ``exact_items``."""
        torch = _torch()
        tau_max, n, T = int(tau_max), int(n), int(T)
        if isinstance(parents, dict):
            ids, count, pcap = parents["ids"], parents["count"], parents["pcap"]
        else:
            K = 2 * tau_max + 1
            pcap = max(1, max((len(p) for p in parents), default=1))
            ids_h = np.zeros((n, pcap), dtype=np.int32)
            cnt_h = np.zeros(n, dtype=np.int32)
            for j, pl in enumerate(parents):
                cnt_h[j] = len(pl)
                for k, (i, neg) in enumerate(pl):
                    ids_h[j, k] = int(i) * K - int(neg)
            ids, count = torch.from_numpy(ids_h).to(self.device), torch.from_numpy(cnt_h).to(self.device)
        shape = (n, n, tau_max + 1)
        val = torch.zeros(shape, dtype=torch.float64, device=self.device)
        dim = torch.zeros(shape, dtype=torch.int32, device=self.device)
        st = torch.zeros(shape, dtype=torch.int32, device=self.device)
        exact = ctypes.c_int64()
        check(self.h, self.lib.pcg_pcmci_mci(self.h, T, n, tau_max, ctypes.c_void_p(ids.data_ptr()),
                                             ctypes.c_void_p(count.data_ptr()), int(pcap), ctypes.c_void_p(val.data_ptr()),
                                             ctypes.c_void_p(dim.data_ptr()), ctypes.c_void_p(st.data_ptr()),
                                             ctypes.byref(exact)), "pcg_pcmci_mci")
        return {"val": val.cpu().numpy(), "dim": dim.cpu().numpy(), "status": st.cpu().numpy(),
                "exact_items": int(exact.value)}

    def pcmci(self, X, tau_max: int, pc_alpha: float) -> dict:
        """``run_pcmci(tau_max, pc_alpha)`` of a T x n array: ``val_matrix`` and ``p_matrix``
        (n x n x (tau_max + 1), [i, j, tau]: column i at lag tau against column j), ``parents`` and
        the counters (``levels``, ``tests`` per target, ``dim_matrix``, ``exact_items`` of PC1 and
        MCI). Raises ``ValueError`` on a constant window or non-finite input."""
        from .graph_construction import pcmci as pm
        par = self.pcmci_parents(X, tau_max, pc_alpha)
        mci = self.pcmci_mci(par["T"], par["n"], par["tau_max"], par)
        pm.raise_on_status(mci["status"])
        val, p = pm.matrices_from_stats(mci["val"], mci["dim"], par["T"] - 2 * par["tau_max"])
        return {"val_matrix": val, "p_matrix": p, "dim_matrix": mci["dim"], "parents": par["parents"],
                "val_min": par["val_min"], "levels": par["levels"], "tests": par["tests"], "status": mci["status"],
                "exact_items": {"parents": par["exact_items"], "mci": mci["exact_items"]}}

    # ------------------------------------------------------------------ fGES
    def fges_limits(self) -> dict:
        """The limits and fast-path guards of the fGES kernels (``pcg_fges_limits``)."""
        from .graph_construction.fges import limits
        return limits()

    def fges_begin(self, X) -> dict:
        """Standardize a T x n array, compute its correlation matrix and keep both in the handle
        for ``fges_gains`` (``pcg_fges_begin``). Host results: ``gain0`` (n x n, the depth-0 gains
        -log1p(-r^2), NaN on the diagonal and on flagged columns) and ``status`` (n: 0, 1 a
        constant column, 2 non-finite)."""
        torch = _torch()
        Xd, T, n, ldx = self._rows(X)
        g0 = torch.empty((max(n, 1), max(n, 1)), dtype=torch.float64, device=self.device)
        st = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        check(self.h, self.lib.pcg_fges_begin(self.h, ctypes.c_void_p(Xd.data_ptr()), T, n, ldx,
                                              ctypes.c_void_p(g0.data_ptr()), ctypes.c_void_p(st.data_ptr())),
              "pcg_fges_begin")
        return {"gain0": g0.cpu().numpy()[:n, :n], "status": st.cpu().numpy()[:n], "T": T, "n": n}

    def fges_gains(self, groups) -> dict:
        """g = log(SSR(y|B) / SSR(y|B + x)) for a batch of groups on the matrix the last
        ``fges_begin`` left in the handle (``pcg_fges_gains``). ``groups``: a list of
        ``(y, B, candidates)`` with B and the candidates sequences of column ids. Host arrays
        ``gain`` and ``status`` (one entry per candidate, in the caller's order; 0 ok, 1 / 2 a
        flagged column, 3 ok by the exact path, 4 refused) and ``exact_items``. The groups are sent
        with the narrow ones (up to ``narrow_max`` candidates) first, as the library asks."""
        from .graph_construction.fges import limits
        narrow_max = limits()["narrow_max"]
        G = len(groups)
        sizes = np.fromiter((len(g[2]) for g in groups), dtype=np.int64, count=G)
        order = np.argsort(sizes > narrow_max, kind="stable")
        sent = [groups[k] for k in order]
        ys = np.fromiter((g[0] for g in sent), dtype=np.int64, count=G)
        boff = np.zeros(G + 1, dtype=np.int64)
        ioff = np.zeros(G + 1, dtype=np.int64)
        np.cumsum([len(g[1]) for g in sent], out=boff[1:])
        np.cumsum(sizes[order], out=ioff[1:])
        nb, ni = int(boff[-1]), int(ioff[-1])
        base = np.fromiter((q for g in sent for q in g[1]), dtype=np.int64, count=nb)
        items = np.fromiter((q for g in sent for q in g[2]), dtype=np.int64, count=ni)
        i32 = np.iinfo(np.int32)
        packed = np.concatenate([ys, boff, ioff, base, items])
        if packed.size and (packed.min() < i32.min or packed.max() > i32.max):
            raise ValueError("fges_gains: an id does not fit int32")
        out = self.fges_gains_csr(ys, boff, base, ioff, items, n_narrow=int((sizes <= narrow_max).sum()))
        # back to the caller's order of groups
        start = np.zeros(G + 1, dtype=np.int64)
        np.cumsum(sizes, out=start[1:])
        back = np.empty(ni, dtype=np.int64)
        for pos, k in enumerate(order):
            back[start[k]:start[k + 1]] = np.arange(ioff[pos], ioff[pos + 1])
        return {"gain": out["gain"][back], "status": out["status"][back], "exact_items": out["exact_items"]}

    def fges_gains_csr(self, grp_y, base_off, base_ids, item_off, item_x, n_narrow, n_base=None, n_items=None) -> dict:
        """``pcg_fges_gains`` on the caller's own CSR arrays (one upload, two result copies):
        groups 0 .. n_narrow - 1 are the narrow ones."""
        torch = _torch()
        parts = [np.ascontiguousarray(a, dtype=np.int32).ravel() for a in (grp_y, base_off, item_off, base_ids, item_x)]
        G = len(parts[0])
        if len(parts[1]) != G + 1 or len(parts[2]) != G + 1:
            raise ValueError("fges_gains: base_off and item_off need one entry more than grp_y")
        nb = len(parts[3]) if n_base is None else int(n_base)
        ni = len(parts[4]) if n_items is None else int(n_items)
        if nb > len(parts[3]) or ni > len(parts[4]):
            raise ValueError("fges_gains: n_base / n_items beyond the arrays")
        dev = torch.from_numpy(np.concatenate(parts + [np.zeros(1, dtype=np.int32)])).to(self.device)
        offs = np.cumsum([0] + [len(p) for p in parts])
        ptr = [ctypes.c_void_p(dev.data_ptr() + 4 * int(o)) for o in offs[:5]]
        gain = torch.empty(max(ni, 1), dtype=torch.float64, device=self.device)
        st = torch.empty(max(ni, 1), dtype=torch.int32, device=self.device)
        exact = ctypes.c_int64()
        check(self.h, self.lib.pcg_fges_gains(self.h, G, ptr[0], ptr[1], ptr[3], nb, ptr[2], ptr[4], ni, int(n_narrow),
                                              ctypes.c_void_p(gain.data_ptr()), ctypes.c_void_p(st.data_ptr()),
                                              ctypes.byref(exact)), "pcg_fges_gains")
        return {"gain": gain.cpu().numpy()[:ni], "status": st.cpu().numpy()[:ni], "exact_items": int(exact.value)}

    # ------------------------------------------------------------------ column scalers
    def scaler_limits(self) -> dict:
        """``lds_rows``: the largest N the in-LDS sort of ``scaler_scores`` takes (``pcg_scaler_limits``)."""
        v = ctypes.c_int64()
        check(self.h, self.lib.pcg_scaler_limits(ctypes.byref(v)), "pcg_scaler_limits")
        return {"lds_rows": int(v.value)}

    def scaler_scores(self, cases, mode) -> list:
        """Per-column scaler fits and scores of many cases in one call (``pcg_scaler_batch``).
        ``cases``: a list of ``(A, B)``, A the N x n normal window and B the M x n anomalous one,
        host arrays or fp64 device tensors (a row-strided device view is read in place). ``mode``:
        0 / "robust" (median, inter-quartile range) or 1 / "standard" (mean, standard deviation).
        Returns per case a dict of the host arrays ``center``, ``scale``, ``score`` (float64) and
        ``status`` (int32: 0 ok, 1 a NaN or Inf in the column, the other three then unspecified),
        n entries each."""
        torch = _torch()
        mode = {"robust": 0, "standard": 1}.get(mode, mode)
        arr = (PcgScalerCase * max(len(cases), 1))()
        keep, offs, off = [], [], 0
        for i, (A, B) in enumerate(cases):
            Ad, N, n, lda = self._rows(A)
            Bd, M, nb, ldb = self._rows(B)
            if nb != n:
                raise ValueError(f"scaler_scores: case {i}: A has {n} columns, B has {nb}")
            keep.append((Ad, Bd))
            arr[i] = PcgScalerCase(Ad.data_ptr(), Bd.data_ptr(), N, M, n, lda, ldb, off)
            offs.append((off, off + n))
            off += n
        vals = torch.empty((3, max(off, 1)), dtype=torch.float64, device=self.device)
        st = torch.empty(max(off, 1), dtype=torch.int32, device=self.device)
        row = vals.stride(0) * 8
        check(self.h, self.lib.pcg_scaler_batch(self.h, arr, len(cases), int(mode),
                                                *(ctypes.c_void_p(vals.data_ptr() + k * row) for k in range(3)),
                                                ctypes.c_void_p(st.data_ptr())), "pcg_scaler_batch")
        v, s = vals.cpu().numpy(), st.cpu().numpy()
        return [{"center": v[0, lo:hi], "scale": v[1, lo:hi], "score": v[2, lo:hi], "status": s[lo:hi]}
                for lo, hi in offs]

    # ------------------------------------------------------------------ K4
    def pagerank_dense(self, A, damping: float = 0.85, n_iter: int = 10, tol: float = 1e-6) -> np.ndarray:
        torch = _torch()
        Ad, lda = self._ld(A)
        m = Ad.shape[0]
        out = torch.empty(m, dtype=torch.float64, device=self.device)
        check(self.h, self.lib.pcg_pagerank_dense(self.h, ctypes.c_void_p(Ad.data_ptr()), m, lda, float(damping),
                                                  int(n_iter), float(tol), ctypes.c_void_p(out.data_ptr())),
              "pcg_pagerank_dense")
        return out.cpu().numpy()

    def pagerank_csr(self, indptr, indices, data, m: int, damping: float = 0.85, n_iter: int = 10,
                     tol: float = 1e-6, nnz: int | None = None) -> np.ndarray:
        """PageRank of a CSR matrix (``pcg_pagerank_csr``); ``nnz`` defaults to len(indices)."""
        torch = _torch()
        ip = torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int32)).to(self.device)
        ix = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(self.device)
        dv = self.to_device(data)
        out = torch.empty(int(m), dtype=torch.float64, device=self.device)
        nnz = len(ix) if nnz is None else int(nnz)
        check(self.h, self.lib.pcg_pagerank_csr(self.h, ctypes.c_void_p(ip.data_ptr()), ctypes.c_void_p(ix.data_ptr()),
                                                ctypes.c_void_p(dv.data_ptr()), int(m), nnz, float(damping),
                                                int(n_iter), float(tol), ctypes.c_void_p(out.data_ptr())),
              "pcg_pagerank_csr")
        return out.cpu().numpy()

    def random_walk_counts(self, P, start: int, num_loop: int, state: int, inc: int) -> np.ndarray:
        torch = _torch()
        Pd, ldp = self._ld(P)
        m = Pd.shape[0]
        counts = torch.empty(m, dtype=torch.int64, device=self.device)
        mask = (1 << 64) - 1
        check(self.h, self.lib.pcg_random_walk(self.h, ctypes.c_void_p(Pd.data_ptr()), m, ldp, int(start),
                                               int(num_loop), (state >> 64) & mask, state & mask,
                                               (inc >> 64) & mask, inc & mask,
                                               ctypes.c_void_p(counts.data_ptr())),
              "pcg_random_walk")
        return counts.cpu().numpy()


def get_engine(device: int | None = None) -> Engine:
    """Process-wide engine for ``device`` (default: LOCAL_RANK or 0)."""
    import os
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    eng = _ENGINES.get(device)
    if eng is None:
        eng = Engine(device)
        _ENGINES[device] = eng
    return eng


def uc_candidates(adj: np.ndarray, sep_xy: np.ndarray, sep_bits: np.ndarray) -> np.ndarray:
    """UCSepset's R0 list (host C++ ``pcg_uc_candidates``): k x 3 int32 (x, y, z)."""
    lib = _lib.load()
    n = adj.shape[0]
    a = np.ascontiguousarray(adj, dtype=np.uint8)
    xy = np.ascontiguousarray(sep_xy, dtype=np.int32)
    bits = np.ascontiguousarray(sep_bits, dtype=np.uint64)
    total = ctypes.c_int64()
    args = (n, a.ctypes.data_as(ctypes.c_void_p), xy.ctypes.data_as(ctypes.c_void_p),
            bits.ctypes.data_as(ctypes.c_void_p), len(xy))
    rc = lib.pcg_uc_candidates(*args, None, 0, ctypes.byref(total))
    if rc != 0:
        raise _lib.PcgError(rc, "pcg_uc_candidates failed")
    out = np.zeros((total.value, 3), np.int32)
    if total.value:
        rc = lib.pcg_uc_candidates(*args, out.ctypes.data_as(ctypes.c_void_p), total.value, ctypes.byref(total))
        if rc != 0:
            raise _lib.PcgError(rc, "pcg_uc_candidates failed")
    return out


def orient_triples(adj: np.ndarray, triples: np.ndarray) -> np.ndarray:
    """Collider step over ``triples`` in the given order, then Meek (``pcg_orient_triples``)."""
    lib = _lib.load()
    n = adj.shape[0]
    a = np.ascontiguousarray(adj, dtype=np.uint8)
    t = np.ascontiguousarray(np.asarray(triples, dtype=np.int32).reshape(-1, 3))
    g = np.zeros((n, n), np.int32)
    rc = lib.pcg_orient_triples(n, a.ctypes.data_as(ctypes.c_void_p), t.ctypes.data_as(ctypes.c_void_p), len(t),
                                g.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        raise _lib.PcgError(rc, "pcg_orient_triples failed")
    return g


def orient(adj: np.ndarray, sep_xy: np.ndarray, sep_bits: np.ndarray, priority: int = 2) -> np.ndarray:
    """Host C++ orientation (UCSepset priority 2 + Meek) → endpoint-code matrix."""
    lib = _lib.load()
    n = adj.shape[0]
    a = np.ascontiguousarray(adj, dtype=np.uint8)
    xy = np.ascontiguousarray(sep_xy, dtype=np.int32)
    bits = np.ascontiguousarray(sep_bits, dtype=np.uint64)
    g = np.zeros((n, n), np.int32)
    rc = lib.pcg_orient(n, a.ctypes.data_as(ctypes.c_void_p), xy.ctypes.data_as(ctypes.c_void_p),
                        bits.ctypes.data_as(ctypes.c_void_p), len(xy), int(priority),
                        g.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        raise _lib.PcgError(rc, f"pcg_orient(priority={priority}) failed")
    return g


def orient_bk(adj: np.ndarray, sep_xy: np.ndarray, sep_bits: np.ndarray, forbidden: np.ndarray,
              required: np.ndarray, priority: int = 2, triples: np.ndarray | None = None,
              scores: np.ndarray | None = None) -> np.ndarray:
    """Orientation with background knowledge (``pcg_orient_bk``): orient_by_background_knowledge,
    then the collider step and Meek, both skipping what the knowledge rules out. Priorities 3/4
    take the candidates' scores (``triples`` in any order); the ordering happens in C++ on the
    candidate order of the oriented graph."""
    lib = _lib.load()
    n = adj.shape[0]
    a = np.ascontiguousarray(adj, dtype=np.uint8)
    xy = np.ascontiguousarray(sep_xy, dtype=np.int32)
    bits = np.ascontiguousarray(sep_bits, dtype=np.uint64)
    fb = np.ascontiguousarray(forbidden, dtype=np.uint8)
    rq = np.ascontiguousarray(required, dtype=np.uint8)
    if fb.shape != (n, n) or rq.shape != (n, n):
        raise ValueError("forbidden / required masks must be n x n")
    t = np.ascontiguousarray(np.asarray(triples if triples is not None else np.zeros((0, 3)), np.int32).reshape(-1, 3))
    sc = np.ascontiguousarray(np.asarray(scores if scores is not None else np.zeros(0), np.float64).reshape(-1))
    if len(sc) != len(t):
        raise ValueError("one score per triple")
    g = np.zeros((n, n), np.int32)
    vp = ctypes.c_void_p
    rc = lib.pcg_orient_bk(n, a.ctypes.data_as(vp), xy.ctypes.data_as(vp), bits.ctypes.data_as(vp), len(xy),
                           int(priority), t.ctypes.data_as(vp), sc.ctypes.data_as(vp), len(t),
                           fb.ctypes.data_as(vp), rq.ctypes.data_as(vp), g.ctypes.data_as(vp))
    if rc != 0:
        raise _lib.PcgError(rc, f"pcg_orient_bk(priority={priority}) failed")
    return g
