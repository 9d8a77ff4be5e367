"""Differentiable wrappers around the HIP kernels (torch.autograd plumbing).

These make the public scoring API (`BaseScoreFunction.score_triple /
score_heads / score_tails`, loss modules) behave like the reference's torch
expressions - callable on embedding tensors, differentiable - while every
number is produced by a kernel of `libbesskge_hip.so`.

The fused training step of `besskge.bess` does not go through autograd at all
(it calls forward and backward kernels explicitly and never builds a dense
gradient); these Functions are the drop-in API surface.
"""

from typing import Any, Optional, Tuple

import torch

from besskge import _native as nat
from besskge._native import RowSource


def _as_rows(x: torch.Tensor, width: int) -> torch.Tensor:
    x = x.reshape(-1, width)
    return x if x.is_contiguous() else x.contiguous()


def _idx32(idx: torch.Tensor) -> torch.Tensor:
    idx = idx.reshape(-1)
    if idx.dtype != torch.int32:
        idx = idx.to(torch.int32)
    return idx if idx.is_contiguous() else idx.contiguous()


class GatherRows(torch.autograd.Function):
    """K1 `table[idx]`; backward = K9 scatter-add into a dense fp32 gradient."""

    @staticmethod
    def forward(ctx: Any, table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:  # type: ignore
        ctx.save_for_backward(idx)
        ctx.table_shape = table.shape
        ctx.table_dtype = table.dtype
        out = nat.gather_rows(table, _idx32(idx))
        return out.reshape(*idx.shape, table.shape[1])

    @staticmethod
    def backward(ctx: Any, g: torch.Tensor) -> Tuple[Optional[torch.Tensor], None]:  # type: ignore
        (idx,) = ctx.saved_tensors
        W = ctx.table_shape[1]
        dense = torch.zeros(ctx.table_shape, dtype=torch.float32, device=g.device)
        nat.scatter_add_rows(dense, _idx32(idx), _as_rows(g.float(), W))
        return dense.to(ctx.table_dtype), None


class ScoreTriple(torch.autograd.Function):
    """K2+K3 positive score of (h, r, t) rows."""

    @staticmethod
    def forward(ctx: Any, desc: nat.ModelDesc, head: torch.Tensor, rel_table: torch.Tensor,  # type: ignore
                rel_idx: torch.Tensor, tail: torch.Tensor) -> torch.Tensor:
        W = desc.width
        h, t, r = _as_rows(head, W), _as_rows(tail, W), _idx32(rel_idx)
        ctx.desc = desc
        ctx.save_for_backward(h, t, rel_table, r)
        ctx.shapes = (head.shape, tail.shape)
        return nat.score_triple_fwd(desc, RowSource(h), RowSource(t), rel_table, r)

    @staticmethod
    def backward(ctx: Any, g: torch.Tensor):  # type: ignore
        h, t, rel_table, r = ctx.saved_tensors
        drel = torch.zeros(rel_table.shape, dtype=torch.float32, device=g.device)
        dh, dt = nat.score_triple_bwd(ctx.desc, RowSource(h), RowSource(t), rel_table, r,
                                      g.float().contiguous(), drel)
        return (None, dh.reshape(ctx.shapes[0]).to(h.dtype), drel.to(rel_table.dtype), None,
                dt.reshape(ctx.shapes[1]).to(t.dtype))


class ScoreNegatives(torch.autograd.Function):
    """K6 + K4/K5: scores of a set of corrupting entities against fixed queries.

    `ent` [S, W] is the entity kept in the triple (tail for corrupted heads,
    head for corrupted tails); `neg` is [B, N, W].  With `sharing` every query
    is scored against all B*N rows (-> [S, B*N]); otherwise B must be S (or 1,
    which broadcasts) and query s is scored against neg[s] (-> [S, N]).
    """

    @staticmethod
    def forward(ctx: Any, desc: nat.ModelDesc, side: int, sharing: bool, ent: torch.Tensor,  # type: ignore
                rel_table: torch.Tensor, rel_idx: torch.Tensor, neg: torch.Tensor) -> torch.Tensor:
        W = desc.width
        x, r = _as_rows(ent, W), _idx32(rel_idx)
        if neg.dim() != 3:
            raise ValueError("negative embeddings must be [B, n_negative, W]")
        B, N = int(neg.shape[0]), int(neg.shape[1])
        S = x.shape[0]
        shared = sharing or B == 1
        if not shared and B != S:
            raise ValueError(f"per-triple negatives need B == batch size ({B} != {S})")
        rows = _as_rows(neg, W)
        q = nat.query_fwd(desc, side, RowSource(x), rel_table, r)
        if shared:
            out = nat.neg_score_shared_fwd(desc, q, RowSource(rows))
        else:
            out = nat.neg_score_pertriple_fwd(desc, q, RowSource(rows), N)
        ctx.desc, ctx.side, ctx.shared, ctx.N = desc, side, shared, N
        ctx.shapes = (ent.shape, neg.shape)
        ctx.save_for_backward(x, rel_table, r, rows, q, out)
        return out

    @staticmethod
    def backward(ctx: Any, g: torch.Tensor):  # type: ignore
        x, rel_table, r, rows, q, out = ctx.saved_tensors
        g = g.float().contiguous()
        if ctx.shared:
            dq, dn = nat.neg_score_shared_bwd(ctx.desc, q, RowSource(rows), out, g)
        else:
            dq, dn = nat.neg_score_pertriple_bwd(ctx.desc, q, RowSource(rows), ctx.N, g)
        drel = torch.zeros(rel_table.shape, dtype=torch.float32, device=g.device)
        dx = nat.query_bwd(ctx.desc, ctx.side, RowSource(x), rel_table, r, dq, drel)
        return (None, None, None, dx.reshape(ctx.shapes[0]).to(x.dtype), drel.to(rel_table.dtype), None,
                dn.reshape(ctx.shapes[1]).to(rows.dtype))


class ReduceNegatives(torch.autograd.Function):
    """K4/K5 alone: scores of candidate rows against a ready-made query matrix
    (the scorers whose query transform is written with torch ops)."""

    @staticmethod
    def forward(ctx: Any, desc: nat.ModelDesc, sharing: bool, query: torch.Tensor, neg: torch.Tensor  # type: ignore
                ) -> torch.Tensor:
        if neg.dim() != 3:
            raise ValueError("negative embeddings must be [B, n_negative, W]")
        B, N = int(neg.shape[0]), int(neg.shape[1])
        S = int(query.shape[0])
        shared = sharing or B == 1
        if not shared and B != S:
            raise ValueError(f"per-triple negatives need B == batch size ({B} != {S})")
        rows = _as_rows(neg, desc.width)
        q = query.float().contiguous()
        out = nat.neg_score_shared_fwd(desc, q, RowSource(rows)) if shared else \
            nat.neg_score_pertriple_fwd(desc, q, RowSource(rows), N)
        ctx.desc, ctx.shared, ctx.N, ctx.neg_shape = desc, shared, N, neg.shape
        ctx.save_for_backward(q, rows, out)
        return out

    @staticmethod
    def backward(ctx: Any, g: torch.Tensor):  # type: ignore
        q, rows, out = ctx.saved_tensors
        g = g.float().contiguous()
        if ctx.shared:
            dq, dn = nat.neg_score_shared_bwd(ctx.desc, q, RowSource(rows), out, g)
        else:
            dq, dn = nat.neg_score_pertriple_bwd(ctx.desc, q, RowSource(rows), ctx.N, g)
        return None, None, dq, dn.reshape(ctx.neg_shape).to(rows.dtype)


class TuckerQuery(torch.autograd.Function):
    """TuckER's query product `(x [S, de], rel_rows [S, dr], core [dr * de, de], swap_axes) -> q [S, de]`
    (`nat.tucker_query_fwd`); the backward gives the three gradients it is asked for.  No double backward."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, rel_rows: torch.Tensor, core: torch.Tensor,  # type: ignore
                swap_axes: bool) -> torch.Tensor:
        x32, r32, c32 = (t.detach().float().contiguous() for t in (x, rel_rows, core))
        ctx.swap = bool(swap_axes)
        ctx.save_for_backward(x32, r32, c32)
        ctx.dtypes = (x.dtype, rel_rows.dtype, core.dtype)
        return nat.tucker_query_fwd(x32, r32, c32, ctx.swap)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx: Any, dq: torch.Tensor):  # type: ignore
        x, rel_rows, core = ctx.saved_tensors
        grads = nat.tucker_query_bwd(x, rel_rows, core, ctx.swap, dq.float().contiguous(), ctx.needs_input_grad[:3])
        return tuple(None if g is None else g.to(dt) for g, dt in zip(grads, ctx.dtypes)) + (None,)


class RelationQuery(torch.autograd.Function):
    """The relation-grouped query product `(x [S, de], M [n_rel, de * de], rel_idx [S], swap_axes) -> q [S, de]`:
    `q[i] = x[i] @ M_r` (`swap_axes`: `M_r @ x[i]`) for the row-major de x de matrix M_r of triple i's relation
    (`nat.relation_query_fwd`).  The batch is grouped by relation once, in the forward; the backward reuses the index
    and computes only the gradients it is asked for (d_M dense, zero for absent relations).  No double backward."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, M: torch.Tensor, rel_idx: torch.Tensor,  # type: ignore
                swap_axes: bool) -> torch.Tensor:
        x32, m32 = (t.detach().float().contiguous() for t in (x, M))
        ctx.seg = nat.SegmentIndex(rel_idx.reshape(-1).to(torch.int32).contiguous(), int(M.shape[0]))
        ctx.swap = bool(swap_axes)
        ctx.save_for_backward(x32, m32)
        ctx.dtypes = (x.dtype, M.dtype)
        return nat.relation_query_fwd(x32, m32, ctx.seg, ctx.swap)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx: Any, dq: torch.Tensor):  # type: ignore
        x, M = ctx.saved_tensors
        grads = nat.relation_query_bwd(x, M, ctx.seg, ctx.swap, dq.float().contiguous(), ctx.needs_input_grad[:2])
        return tuple(None if g is None else g.to(dt) for g, dt in zip(grads, ctx.dtypes)) + (None, None)


class StructuredQuery(torch.autograd.Function):
    """The query of a structured bilinear scorer `(desc, side, rows [S, W], rel_table [n_rel, Wr], rel_idx [S]) ->
    q [S, W]` for the term table `desc` (`nat.struct_query_fwd`); rows and relation table are of the table type, the
    gradients come back in their dtypes (the relation table's dense, zero for absent relations).  No double backward."""

    @staticmethod
    def forward(ctx: Any, desc: nat.StructDesc, side: int, rows: torch.Tensor, rel_table: torch.Tensor,  # type: ignore
                rel_idx: torch.Tensor) -> torch.Tensor:
        x, r = _as_rows(rows.detach(), rows.shape[-1]), _idx32(rel_idx)
        ctx.desc, ctx.side, ctx.shape = desc, side, rows.shape
        ctx.save_for_backward(x, rel_table.detach(), r)
        return nat.struct_query_fwd(desc, side, RowSource(x), rel_table.detach(), r)[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx: Any, dq: torch.Tensor):  # type: ignore
        x, rel_table, r = ctx.saved_tensors
        d_rel = torch.zeros(rel_table.shape, dtype=torch.float32, device=dq.device) if ctx.needs_input_grad[3] else None
        dx, _ = nat.struct_query_bwd(ctx.desc, ctx.side, RowSource(x), rel_table, r, dq.float().contiguous(), d_rel)
        return None, None, dx.reshape(ctx.shape).to(x.dtype), None if d_rel is None else d_rel.to(rel_table.dtype), None


class BoxEQuery(torch.autograd.Function):
    """BoxE's S-row work `(desc, side, eps, rows [S, 2 d], rel_table [n_rel, 4 d + 2], rel_idx [S], other [S, 2 d] |
    None)`: the query `q [S, 6 d]` of the kept `rows` without `other`, the triples' scores `[S]` with it
    (`nat.boxe_query_fwd`).  Rows and relation table are of the table type, the gradients come back in their dtypes
    (the relation table's dense, zero for absent relations).  No double backward."""

    @staticmethod
    def forward(ctx: Any, desc: nat.ModelDesc, side: int, eps: float, rows: torch.Tensor,  # type: ignore
                rel_table: torch.Tensor, rel_idx: torch.Tensor, other: Optional[torch.Tensor]) -> torch.Tensor:
        W = rows.shape[-1]
        x, r = _as_rows(rows.detach(), W), _idx32(rel_idx)
        o = None if other is None else _as_rows(other.detach(), W)
        ctx.desc, ctx.side, ctx.eps, ctx.shape, ctx.scores = desc, side, eps, rows.shape, other is not None
        ctx.save_for_backward(x, rel_table.detach(), r, *(() if o is None else (o,)))
        q, pos = nat.boxe_query_fwd(desc, side, eps, RowSource(x), rel_table.detach(), r,
                                    other=None if o is None else RowSource(o), want_query=o is None)
        return q if o is None else pos.reshape(rows.shape[:-1])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx: Any, g: torch.Tensor):  # type: ignore
        x, rel_table, r = ctx.saved_tensors[:3]
        o = ctx.saved_tensors[3] if ctx.scores else None
        d_rel = torch.zeros(rel_table.shape, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[4] else None
        g = g.float().contiguous()
        dx, do = nat.boxe_query_bwd(ctx.desc, ctx.side, ctx.eps, RowSource(x), rel_table, r, None if ctx.scores else g,
                                    d_rel, other=None if o is None else RowSource(o),
                                    d_pos=g.reshape(-1) if ctx.scores else None)
        return (None, None, None, dx.reshape(ctx.shape).to(x.dtype), None if d_rel is None else d_rel.to(rel_table.dtype),
                None, None if do is None else do.reshape(ctx.shape).to(o.dtype))


class ConvEQuery(torch.autograd.Function):
    """ConvE's conv + channel affine + ReLU + channel mask + FC product `(x [S, Cin, H2, W], K [Cout, Cin, kh, kw],
    a [Cout], b [Cout], m [S, Cout] | None, Wfc [d, F]) -> y [S, d]` (`nat.conve_query_fwd`): the `[S, F]` feature map
    is never written, forward or backward.  The backward gives the gradients it is asked for (`m` gets none).  No
    double backward."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, K: torch.Tensor, a: torch.Tensor, b: torch.Tensor,  # type: ignore
                m: Optional[torch.Tensor], Wfc: torch.Tensor) -> torch.Tensor:
        ops32 = [None if t is None else t.detach().float().contiguous() for t in (x, K, a, b, m, Wfc)]
        ctx.has_mask = m is not None
        ctx.save_for_backward(*(t for t in ops32 if t is not None))
        ctx.dtypes = (x.dtype, K.dtype, a.dtype, b.dtype, Wfc.dtype)
        return nat.conve_query_fwd(*ops32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx: Any, dy: torch.Tensor):  # type: ignore
        saved = list(ctx.saved_tensors)
        x, K, a, b = saved[:4]
        m, Wfc = (saved[4] if ctx.has_mask else None), saved[-1]
        need = ctx.needs_input_grad
        d_Wfc, d_x, d_K, d_a, d_b = nat.conve_query_bwd(x, K, a, b, m, Wfc, dy.float().contiguous(),
                                                        (need[5], need[0], need[1], need[2], need[3]))
        grads = [None if g is None else g.to(dt) for g, dt in zip((d_x, d_K, d_a, d_b, d_Wfc), ctx.dtypes)]
        return grads[0], grads[1], grads[2], grads[3], None, grads[4]


class ConvEChannelStats(torch.autograd.Function):
    """Training-mode batch statistics of `conv2d(x, K)` per output channel without the feature map:
    `(x, K) -> (mean [Cout], M2 [Cout])`, M2 the centred sum of squares (`nat.conve_stats_fwd`).  No double backward."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, K: torch.Tensor):  # type: ignore
        x32, k32 = x.detach().float().contiguous(), K.detach().float().contiguous()
        mean, M2 = nat.conve_stats_fwd(x32, k32)
        ctx.save_for_backward(x32, k32, mean)
        ctx.dtypes = (x.dtype, K.dtype)
        return mean, M2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx: Any, d_mean: torch.Tensor, d_M2: torch.Tensor):  # type: ignore
        x, K, mean = ctx.saved_tensors
        grads = nat.conve_stats_bwd(x, K, mean, d_mean.float().contiguous(), d_M2.float().contiguous(),
                                    ctx.needs_input_grad[:2])
        return tuple(None if g is None else g.to(dt) for g, dt in zip(grads, ctx.dtypes))


class Loss(torch.autograd.Function):
    """K8 fused loss + score gradients (`logq`: the sampled softmax's per-candidate log-proposals, see
    `nat.loss_fwd_bwd`)."""

    @staticmethod
    def forward(ctx: Any, ldesc: nat.LossDesc, pos: torch.Tensor, neg: torch.Tensor,  # type: ignore
                weight: torch.Tensor, logq: Optional[torch.Tensor] = None) -> torch.Tensor:
        need = pos.requires_grad or neg.requires_grad
        loss, dp, dn = nat.loss_fwd_bwd(ldesc, pos.contiguous(), neg.contiguous(),
                                        weight.reshape(-1).float().contiguous(), True, logq=logq)
        ctx.save_for_backward(dp, dn)
        del need
        return loss

    @staticmethod
    def backward(ctx: Any, g: torch.Tensor):  # type: ignore
        dp, dn = ctx.saved_tensors
        return None, g * dp, g * dn, None, None
