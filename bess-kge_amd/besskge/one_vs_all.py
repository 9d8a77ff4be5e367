"""1vsAll training: the loss of a triple is the cross entropy of its true
completion against EVERY entity of the graph (Lacroix et al.'s ComplEx-N3
recipe, LibKGE's "1vsAll", PyKEEN's LCWA) - without the `[S, n_entity]` score
matrix.

For a micro-batch of S triples of a replica and corruption scheme "t" ("h" is
the mirror image):

    loss = loss_scale * sum_i w_i * ( log sum_{e real} exp(score(q_i, e)) - pos_i )

`e` runs over every real entity of every shard (pad rows, local index >=
`sharding.shard_counts[shard]`, are never candidates); the true tail is one of
them, nothing is masked; `pos_i` is `score_triple`; `w_i` = triple_weight x
triple_mask.  That is `SampledSoftmaxCrossEntropyLoss` over "all other
entities" (N = n_entity - 1, shift 0).

Data flow (ScoreMoving's): every shard scores the queries of all replicas
against its own rows, but what travels back is two floats per (query, shard):

  forward   own query-side rows gathered, rows + relation ids all-gathered,
            `query_fwd` -> [n * S, W]; `nat.neg_score_shared_lse` over the
            shard's real rows -> (m, l) per query; all-to-all of those partials
            to the triples' owners, merged there in shard order -> lse [S];
            positive tails exchanged as in EmbeddingMoving, `score_triple`.
  backward  (lse, coef = loss_scale * w * grad_scale) all-gathered;
            `nat.neg_score_shared_bwd_softmax` on every shard gives the dense
            gradient of its own rows [M_real, W] (no row gradient crosses the
            link) and its share of d_query, which goes to the owners by
            all-to-all and is summed in shard order; `query_bwd`, `triple_bwd`
            with d_pos = -coef, the regulariser on the positives' rows.
  update    everything is handed to `BessKGE._hand_over` as `_ShardGrads`:
            the dense gradient is the row list (arange(M_real), d_neg) beside
            the head / tail lists, so every optimiser, update route and
            gradient accumulation work as they do for the other schemes.
"""

from typing import Any, Dict, List, Optional

import torch

from besskge import _native as nat
from besskge._native import RowSource
from besskge.bess import BessKGE, _Batch, _PendingUpdate, _ReplicaStep, _ShardGrads, _StepContext, _i32
from besskge.loss import BaseLossFunction, SampledSoftmaxCrossEntropyLoss
from besskge.negative_sampler import PlaceholderNegativeSampler, ShardedNegativeSampler
from besskge.regularizer import EmbeddingRegularizer
from besskge.scoring import BaseScoreFunction, ComplEx, DistMult, RotatE, TransE


class OneVsAllBessKGE(BessKGE):
    """Training step whose negatives are all entities (see the module docstring).  Eager only."""

    def __init__(
        self,
        negative_sampler: ShardedNegativeSampler,
        score_fn: BaseScoreFunction,
        loss_fn: BaseLossFunction,
        evaluation: Optional[Any] = None,
        regularizer: Optional[EmbeddingRegularizer] = None,
        return_scores: bool = False,
    ) -> None:
        """
        :param negative_sampler: `PlaceholderNegativeSampler("h" | "t")` (nothing is sampled).
        :param score_fn: TransE, RotatE, DistMult or ComplEx.
        :param loss_fn: `SampledSoftmaxCrossEntropyLoss(n_entity=sharding.n_entity)`
            without `proposal_correction`; only its `loss_scale` enters.
        :param evaluation: must be None (ranks over all entities: `AllScoresPipeline`).
        :param regularizer: as for the other schemes.
        """
        if return_scores:
            raise ValueError("OneVsAllBessKGE never holds the [S, n_entity] scores: return_scores=True is refused")
        if not isinstance(negative_sampler, PlaceholderNegativeSampler) or negative_sampler.corruption_scheme not in (
                "h", "t"):
            raise ValueError('OneVsAllBessKGE takes PlaceholderNegativeSampler("h") or ("t"): every entity is a '
                             'candidate, nothing is sampled (scheme "ht" is not built)')
        if type(score_fn) not in (TransE, RotatE, DistMult, ComplEx):
            raise ValueError("OneVsAllBessKGE: TransE, RotatE, DistMult or ComplEx "
                             f"(the scorers of bess_neg_score_shared_fwd_lse), not {type(score_fn).__name__}")
        if not isinstance(loss_fn, SampledSoftmaxCrossEntropyLoss) or loss_fn.proposal_correction \
                or int(loss_fn.n_entity) != int(score_fn.sharding.n_entity):
            raise ValueError("OneVsAllBessKGE: the loss is SampledSoftmaxCrossEntropyLoss(n_entity=sharding.n_entity) "
                             "without proposal_correction (the softmax runs over all entities: nothing to correct)")
        if evaluation is not None:
            raise ValueError("OneVsAllBessKGE: metrics over all entities come from AllScoresPipeline, evaluation=None")
        super().__init__(negative_sampler, score_fn, loss_fn, None, False, False, regularizer)

    # ------------------------------------------------------------------ pieces
    def _triple_weight(self, batch: _Batch, device: torch.device, scale: float = 1.0) -> torch.Tensor:
        """triple_weight x triple_mask (x the gradient scale): a masked triple is no term of the loss."""
        w = super()._triple_weight(batch, device, scale)
        tm = batch.get("triple_mask")
        if tm is None:
            return w
        return (w * tm.reshape(-1).to(device=device, dtype=torch.float32)).contiguous()

    def _candidates(self, shard: int, table: torch.Tensor) -> RowSource:
        """The shard's real rows (pad rows behind them are no entities)."""
        return RowSource(table[: int(self.sharding.shard_counts[shard])])

    def score_batch_replicas(self, batches: List[_Batch], ctx: Optional[_StepContext] = None) -> List[_ReplicaStep]:
        raise RuntimeError("OneVsAllBessKGE holds no score matrix; scores over all entities: AllScoresBESS")

    def _forward(self, batches: List[_Batch], scale: float) -> Dict[str, Any]:
        group = self._group()
        n = group.n_shard
        fn = self.score_fn
        W = self.entity_embedding_size
        desc = fn.kernel_desc()
        scheme = self.negative_sampler.corruption_scheme
        side = nat.CORRUPT_HEAD if scheme == "h" else nat.CORRUPT_TAIL
        if len(batches) != len(group.local_shards):
            raise ValueError(f"{len(batches)} batches for {len(group.local_shards)} local replicas")
        steps: List[_ReplicaStep] = []
        tails_out, rows_q, rels = [], [], []
        for shard, b in zip(group.local_shards, batches):
            st = _ReplicaStep()
            st.table = self._local_table(shard)
            dev = st.table.device
            if nat._capturing(dev):
                raise RuntimeError("OneVsAllBessKGE runs eagerly: its step reads a flag on the host and cannot be "
                                   "recorded into a graph (Options.use_graphs / use_plans)")
            for k in ("head", "relation", "tail"):
                if b[k].shape[0] != 1:
                    raise ValueError(f"`{k}` must have a leading replica dim of 1, got {tuple(b[k].shape)}")
            head, rel, tail = (_i32(b[k].squeeze(0)).to(dev) for k in ("head", "relation", "tail"))
            st.n, st.ppp = n, int(head.shape[1])
            st.head_idx, st.rel_idx = head.reshape(-1), rel.reshape(-1)
            st.local_tail, st.sm_head = tail, head
            # rows of my shard that other replicas need: the tails of their triples
            tail_rows = nat.gather_rows(st.table, tail.reshape(-1)).reshape(n, st.ppp, W)
            tails_out.append(tail_rows)
            rows_q.append(tail_rows if scheme == "h" else nat.gather_rows(st.table, st.head_idx).reshape(n, st.ppp, W))
            rels.append(rel)
            steps.append(st)
        rel_all = group.all_gather(rels)  # [n(j), n, ppp]
        rows_all = group.all_gather(rows_q)  # "t": [n(j), n(t), ppp, W]; "h": [n(t), n(j), ppp, W]
        partials, q_state = [], []
        for shard, st, rows, relr in zip(group.local_shards, steps, rows_all, rel_all):
            dev = st.table.device
            idx = None
            if scheme == "h":  # gathered as [t, j, p] but wanted as [j, t, p]
                idx = self._static_map(
                    ("smT", n, st.ppp),
                    lambda: torch.arange(n * n * st.ppp).reshape(n, n, st.ppp).transpose(0, 1).reshape(-1), dev)
            ent = RowSource(rows.reshape(-1, W), idx)
            rel_q = relr.reshape(-1).contiguous()
            query, qctx = fn.query_fwd(side, ent, rel_q)
            state = nat.neg_score_shared_lse(desc, query, self._candidates(shard, st.table))
            partials.append(state.reshape(n, n * st.ppp, 2))
            q_state.append((ent, rel_q, query, qctx))
        ml_back = group.all_to_all(partials)  # [n(shard), S, 2] at the triples' owner
        tails_in = group.all_to_all(tails_out)
        outs, lses, coefs = [], [], []
        for st, b, ml, tl in zip(steps, batches, ml_back, tails_in):
            dev = st.table.device
            # the n partials of a query, merged in shard order
            m, l = ml[0, :, 0], ml[0, :, 1]
            for s in range(1, n):
                mm = torch.maximum(m, ml[s, :, 0])
                l = l * torch.exp(m - mm) + ml[s, :, 1] * torch.exp(ml[s, :, 0] - mm)
                m = mm
            lse = (m + torch.log(l)).contiguous()
            st.recv = tl.reshape(-1, W)
            st.tail = RowSource(st.recv, None)
            st.positive_score, st.triple_ctx = fn.triple_fwd(RowSource(st.table, st.head_idx), st.tail, st.rel_idx)
            w = self._triple_weight(b, dev, scale)
            coef = (w * float(self.loss_fn.loss_scale)).expand(lse.shape[0]).contiguous()
            loss = (coef * (lse - st.positive_score)).sum().reshape(1)
            out: Dict[str, Any] = dict(loss=(loss if scale == 1.0 else loss / scale).reshape(()),
                                       positive_score=st.positive_score.to(fn.relation_embedding.dtype))
            outs.append(out)
            lses.append(lse)
            coefs.append(coef)
        return dict(steps=steps, q_state=q_state, outs=outs, lse=lses, coef=coefs)

    # ---------------------------------------------------------------- forward
    def forward(self, head: torch.Tensor, relation: torch.Tensor, tail: torch.Tensor,  # type: ignore[override]
                negative: Optional[torch.Tensor] = None, triple_mask: Optional[torch.Tensor] = None,
                triple_weight: Optional[torch.Tensor] = None, **unused: Any) -> Dict[str, Any]:
        batch = dict(head=head, relation=relation, tail=tail)
        for k, v in (("triple_mask", triple_mask), ("triple_weight", triple_weight)):
            if v is not None:
                batch[k] = v
        if len(self._group().local_shards) != 1:
            raise RuntimeError("forward() steps a single replica; use forward_replicas()")
        return self.forward_replicas([batch])[0]

    def forward_replicas(self, batches: List[_Batch]) -> List[Dict[str, Any]]:
        fwd = self._forward(batches, 1.0)
        if self.regularizer is not None:
            for st, b, out in zip(fwd["steps"], batches, fwd["outs"]):
                self._regularize(st, b, out)  # (the value only)
        return fwd["outs"]

    # ---------------------------------------------------------------- training
    def train_step_replicas(self, batches: List[_Batch], optimizer: Any, pending: Optional[List[_PendingUpdate]] = None,
                            grad_scale: float = 1.0) -> List[Dict[str, Any]]:
        """Forward + backward + update of one micro-batch (`pending`, `grad_scale`: as for the other schemes)."""
        group = self._group()
        n = group.n_shard
        fn = self.score_fn
        W = self.entity_embedding_size
        desc = fn.kernel_desc()
        scheme = self.negative_sampler.corruption_scheme
        side = nat.CORRUPT_HEAD if scheme == "h" else nat.CORRUPT_TAIL
        fwd = self._forward(batches, grad_scale)
        steps, outs = fwd["steps"], fwd["outs"]
        ctx = _StepContext(batches, training=True, grad_scale=grad_scale)
        d_rel = self._relation_gradient(ctx, pending)
        shards = [_ShardGrads(st) for st in steps]
        # positives: d loss / d pos = -coef
        d_tails = []
        for sh, b, out, coef in zip(shards, batches, outs, fwd["coef"]):
            st = sh.step
            dh, dt = fn.triple_bwd(RowSource(st.table, st.head_idx), st.tail, st.rel_idx, st.triple_ctx,
                                   (-coef).contiguous(), d_rel)
            if self.regularizer is not None:
                self._regularize(st, b, out, grad_scale, dh, dt, d_rel)
            sh.rows.append((st.head_idx, dh))
            d_tails.append(dt.reshape(n, st.ppp, W))
        d_tail_back = group.all_to_all(d_tails)
        # the softmax: every shard needs (lse, coef) of the queries it scored
        norm_all = group.all_gather([torch.stack([z, c], dim=1) for z, c in zip(fwd["lse"], fwd["coef"])])  # [n(j), S, 2]
        d_q = []
        for shard, sh, dtb, norm, (ent, rel_q, query, qctx) in zip(group.local_shards, shards, d_tail_back, norm_all,
                                                                  fwd["q_state"]):
            st = sh.step
            dev = st.table.device
            sh.rows.append((st.local_tail.reshape(-1), dtb.reshape(-1, W)))
            norm = norm.reshape(-1, 2)
            cand = self._candidates(shard, st.table)
            dq, dn = nat.neg_score_shared_bwd_softmax(desc, query, cand, norm[:, 0].contiguous(),
                                                      norm[:, 1].contiguous())
            rows = self._static_map(("1vsall rows", len(cand)), lambda: torch.arange(len(cand)), dev)
            sh.rows.append((rows, dn))
            dx = fn.query_bwd(side, ent, rel_q, qctx, dq, d_rel)
            if ent.idx is not None:  # undo the [t, j, p] -> [j, t, p] re-ordering
                buf = torch.empty_like(dx)
                buf[ent.idx.long()] = dx
                dx = buf
            d_q.append(dx.reshape(n, -1, W))
        # the shards' shares of the query gradients to the owners of the query-side rows, summed in shard order
        for sh, back in zip(shards, group.all_to_all(d_q)):
            st = sh.step
            total = back[0]
            for s in range(1, n):
                total = total + back[s]
            own = st.local_tail.reshape(-1) if scheme == "h" else st.head_idx
            sh.rows.append((own, total.reshape(-1, W).contiguous()))
        self._hand_over(shards, d_rel, optimizer, desc, pending)
        return outs
