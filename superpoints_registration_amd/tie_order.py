"""Neighbour ties in the reference's order (tie_order='reference'; csrc/tie_order.h, include/spr.h).

The table search orders a row by (d2, index).  The reference's rows -- batch_nanoflann_neighbors, neighbors.cpp:211-332
-- order an equal-d2 run by the kd-tree's visit order passed through an unstable std::sort.  That order is a function of
the cloud's supports and the query; the library replays it.  ReplayTree holds the kd-tree replay of one support set
(built once per pyramid level and shared by the conv, pool and up-sampling searches against it, like ops.RadiusTable;
it does not depend on the radius); apply() rewrites, in place, the rows of a matrix in which an equal-d2 run touches
the kept columns.  The default, tie_order='index', never comes here.
"""
import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, ops

TIE_ORDERS = ('index', 'reference')


def check(tie_order, select=None) -> str:
    """Validates the option (and its combination with a selection rule); returns it."""
    if tie_order not in TIE_ORDERS:
        raise ValueError(f"tie_order must be 'index' or 'reference', got {tie_order!r}")
    if tie_order == 'reference' and select in (ops.SELECT_INDEX, 'index'):
        raise ValueError("tie_order='reference' orders equal-distance runs of neighbor_select='nearest' rows; "
                         "neighbor_select='index' rows are ordered by index and have no ties")
    return tie_order


class TieStatus(tuple):
    """(rows_fixed, set_mismatch, overflow, error) of one fix-up, with the matrix's row count."""
    rows = 0
    rows_fixed = property(lambda s: s[0])
    set_mismatch = property(lambda s: s[1])


def _status(words, rows, what) -> TieStatus:
    st = TieStatus(int(v) for v in words)
    st.rows = int(rows)
    if st[3]:
        raise RuntimeError(f"{what}: the kd-tree replay does not belong to these supports, failed to build, or is "
                           "deeper than the depth passed")
    if st[2]:
        raise RuntimeError(f"{what}: {st[2]} rows did not fit the scratch sized from max_count and the tree's depth")
    if st[1]:
        raise RuntimeError(f"{what}: the replayed search disagrees with the table search on {st[1]} rows "
                           "(set_mismatch); they were left in index order")
    return st


class ReplayTree:
    """kd-tree replay of one support set (spr_kdtree_replay_build): one device->host read of its depth."""

    def __init__(self, supports: torch.Tensor, s_cu: torch.Tensor):
        self.supports = ops._dev(supports, "supports", torch.float32)
        self.s_cu = ops._dev(s_cu, "s_cu", torch.int32)
        self.ns, self.nb = self.supports.shape[0], self.s_cu.numel() - 1
        L = _lib.lib()
        self.blob = torch.empty((L.spr_kdtree_replay_size(self.ns, self.nb),), dtype=torch.uint8,
                                device=self.supports.device)
        _lib.check(L.spr_kdtree_replay_build(ops._ptr(self.supports), ops._ptr(self.s_cu), self.ns, self.nb,
                                             ops._ptr(self.blob), self.blob.numel(), ops._stream(self.supports)),
                   "spr_kdtree_replay_build")
        head = self.blob[:8].view(torch.int32).tolist()
        if head[1]:
            raise RuntimeError("spr_kdtree_replay_build: s_cu is not a prefix of cloud lengths, or a cloud's tree needs "
                               "more than two nodes per point (non-finite coordinates)")
        self.depth = head[0]
        self._built = (ops._ident(self.supports), ops._ident(self.s_cu))
        self.last = None            # TieStatus of the latest apply()

    def matches(self, supports: torch.Tensor, s_cu: torch.Tensor) -> bool:
        return ((ops._ident(supports), ops._ident(s_cu)) == self._built
                and (ops._ident(self.supports), ops._ident(self.s_cu)) == self._built and supports.shape[0] == self.ns)

    def scratch_bytes(self, nq: int, max_count: int) -> int:
        return _lib.lib().spr_tie_order_workspace_size(int(nq), int(max_count), self.depth)

    def apply(self, nbr: torch.Tensor, queries: torch.Tensor, q_cu: torch.Tensor, radius: float,
              max_count: int) -> TieStatus:
        """nbr: the int32 [Nq, W] matrix a nearest-rule search returned (a column slice of its [Nq, limit] storage is
        fine), max_count its untruncated widest row.  Rewritten in place; one device->host read of the status."""
        queries = ops._dev(queries, "queries", torch.float32)
        q_cu = ops._dev(q_cu, "q_cu", torch.int32)
        if (not nbr.is_cuda or nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != queries.shape[0]
                or (nbr.shape[1] and nbr.stride(1) != 1)):
            raise ValueError("tie_order.apply: nbr must be an int32 [Nq, W] device matrix with unit column stride")
        nq, width = nbr.shape
        stride = max(nbr.stride(0), width)      # (a one-row view may report any row stride)
        L = _lib.lib()
        ws = ops._workspace(self.scratch_bytes(nq, max_count), queries.device)
        st = torch.empty((4,), dtype=torch.int32, device=queries.device)
        _lib.check(L.spr_tie_order(ops._ptr(queries), ops._ptr(q_cu), nq, ops._ptr(self.supports), ops._ptr(self.s_cu),
                                   self.ns, self.nb, float(radius), ops._ptr(self.blob), self.depth, ops._ptr(nbr),
                                   int(stride), int(width), int(max_count), ops._ptr(st), ops._ptr(ws), ws.numel(),
                                   ops._stream(queries)), "spr_tie_order")
        self.last = _status(st.tolist(), nq, "spr_tie_order")
        return self.last


def apply(nbr: torch.Tensor, queries: torch.Tensor, q_cu: torch.Tensor, supports: torch.Tensor, s_cu: torch.Tensor,
          radius: float, max_count: int, tree: Optional[ReplayTree] = None) -> TieStatus:
    """One-off form: builds the supports' tree unless one is passed."""
    if tree is None or not tree.matches(supports, s_cu):
        tree = ReplayTree(supports, s_cu)
    return tree.apply(nbr, queries, q_cu, radius, max_count)


# ---- host twins (numpy; the same header code, no device) ----------------------------------------------------------------
def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _cu(lengths):
    cu = np.zeros(len(lengths) + 1, np.int32)
    cu[1:] = np.cumsum(np.asarray(lengths, dtype=np.int64))
    return cu


def apply_host(nbr, queries, supports, q_lengths, s_lengths, radius: float, max_count: int) -> Tuple[np.ndarray, TieStatus]:
    """spr_tie_order_host on numpy arrays: (the [Nq, W] matrix with ties in the reference's order, its status).  nbr:
    rows of the nearest rule in (d2, index) order, shadow = Ns."""
    out = _np(nbr, np.int32).copy()
    q, s = _np(queries, np.float32), _np(supports, np.float32)
    q_cu, s_cu = _cu(q_lengths), _cu(s_lengths)
    nq, width = out.shape
    st = np.zeros(4, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(_lib.lib().spr_tie_order_host(p(q), p(q_cu), nq, p(s), p(s_cu), s.shape[0], len(s_lengths), float(radius),
                                             p(out), max(width, 1), width, int(max_count), p(st)),
               "spr_tie_order_host")
    return out, _status(st, nq, "spr_tie_order_host")


def std_sort_replay(keys) -> Tuple[np.ndarray, int]:
    """(the order std::sort leaves the pairs (i, keys[i]) in when it compares the keys only, the number of ranges
    that ran out of depth and were heap-sorted)."""
    k = _np(keys, np.float32)
    perm = np.zeros(k.shape[0], np.int32)
    heap = ctypes.c_int(0)
    _lib.check(_lib.lib().spr_std_sort_replay_host(k.ctypes.data_as(ctypes.c_void_p), k.shape[0],
                                                   perm.ctypes.data_as(ctypes.c_void_p), ctypes.byref(heap)),
               "spr_std_sort_replay_host")
    return perm, int(heap.value)
