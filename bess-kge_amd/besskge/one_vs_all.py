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
  relation prediction (`relation_prediction_weight` > 0; Chen et al. 2021; DistMult / ComplEx): every triple also
            pays weight * coef_i * (log sum_{r' < n_relation} exp(score(h_i, r', t_i)) - pos_i).  The owner of the
            triples holds both rows already: `nat.relation_lse_fwd` right after `triple_fwd`,
            `nat.relation_lse_bwd` right after `triple_bwd`, added into the same dh, dt and d_rel - nothing new
            crosses the link.
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
from besskge.scoring import (RESCAL, BaseScoreFunction, ComplEx, ConvE, DistMult, RotatE, StructuredBilinear, TransE,
                             TuckER)


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
        relation_prediction_weight: float = 0.0,
    ) -> None:
        """
        :param negative_sampler: `PlaceholderNegativeSampler("h" | "t")` (nothing is sampled).
        :param score_fn: TransE, RotatE, DistMult or ComplEx; or TuckER / RESCAL / ConvE / StructuredBilinear (their
            query against DistMult's kernels; ConvE on either query route, tails only: `[embedding | bias]` rows against `[q | 1]`).
        :param loss_fn: `SampledSoftmaxCrossEntropyLoss(n_entity=sharding.n_entity)`
            without `proposal_correction`; only its `loss_scale` enters.
        :param evaluation: must be None (ranks over all entities: `AllScoresPipeline`).
        :param regularizer: as for the other schemes.
        :param relation_prediction_weight: weight of the cross entropy of every triple's relation against all
            rows of the relation table (inverse relations included), DistMult and ComplEx only; 0: no such term.
        """
        me = type(self).__name__
        self.relation_prediction_weight = float(relation_prediction_weight)
        if not self.relation_prediction_weight >= 0.0:
            raise ValueError(f"{me}: relation_prediction_weight must be >= 0, got {relation_prediction_weight}")
        if self.relation_prediction_weight > 0.0 and type(score_fn) not in (DistMult, ComplEx):
            raise ValueError(f"{me}: relation prediction needs a score that is a dot product with the relation row: "
                             f"DistMult or ComplEx, not {type(score_fn).__name__}")
        if return_scores:
            raise ValueError(f"{me} never holds the [S, n_entity] scores: return_scores=True is refused")
        if not isinstance(negative_sampler, PlaceholderNegativeSampler) or negative_sampler.corruption_scheme not in (
                "h", "t"):
            raise ValueError(f'{me} takes PlaceholderNegativeSampler("h") or ("t"): every entity is a '
                             'candidate, nothing is sampled (scheme "ht" is not built)')
        if type(score_fn) not in (TransE, RotatE, DistMult, ComplEx, TuckER, RESCAL, ConvE, StructuredBilinear):
            raise ValueError(f"{me}: TransE, RotatE, DistMult or ComplEx "
                             f"(the scorers of bess_neg_score_shared_fwd_lse; TuckER, RESCAL, ConvE and StructuredBilinear through "
                             f"DistMult's), "
                             f"not {type(score_fn).__name__}")
        if type(score_fn) is ConvE and negative_sampler.corruption_scheme == "h":
            raise NotImplementedError("ConvE should not be used with head corruption")
        self._check_loss(loss_fn, score_fn)
        if evaluation is not None:
            raise ValueError(f"{me}: metrics over all entities come from AllScoresPipeline, evaluation=None")
        super().__init__(negative_sampler, score_fn, loss_fn, None, False, False, regularizer)

    # ---- what a loss over all entities defines (KvsAllBessKGE overrides these five) ----------------------------
    def _check_loss(self, loss_fn: BaseLossFunction, score_fn: BaseScoreFunction) -> None:
        if not isinstance(loss_fn, SampledSoftmaxCrossEntropyLoss) or loss_fn.proposal_correction \
                or int(loss_fn.n_entity) != int(score_fn.sharding.n_entity):
            raise ValueError("OneVsAllBessKGE: the loss is SampledSoftmaxCrossEntropyLoss(n_entity=sharding.n_entity) "
                             "without proposal_correction (the softmax runs over all entities: nothing to correct)")

    def _query_labels(self, steps: List[_ReplicaStep], rel_all: List[torch.Tensor]) -> List[Any]:
        """Per local shard: what its pass over all queries needs beside the query matrix (nothing here)."""
        return [None] * len(steps)

    def _shard_partial(self, shard: int, st: _ReplicaStep, desc: Any, query: torch.Tensor, labels: Any) -> torch.Tensor:
        """[n_query, k] f32: the shard's share of every query's sum over all entities - here (m, l)."""
        return nat.neg_score_shared_lse(desc, query, self._candidates(shard, st.table))

    def _merge_partials(self, part: torch.Tensor, pos: torch.Tensor) -> Any:
        """part [n_shard, S, k] at the triples' owner -> (what the backward needs of every row [S, m], the rows'
        loss terms [S], d term / d pos); merged in shard order."""
        m, l = part[0, :, 0], part[0, :, 1]
        for s in range(1, part.shape[0]):
            mm = torch.maximum(m, part[s, :, 0])
            l = l * torch.exp(m - mm) + part[s, :, 1] * torch.exp(part[s, :, 0] - mm)
            m = mm
        lse = (m + torch.log(l)).contiguous()
        return lse.reshape(-1, 1), lse - pos, -1.0

    def _shard_backward(self, shard: int, st: _ReplicaStep, desc: Any, query: torch.Tensor, norm: torch.Tensor,
                        coef: torch.Tensor, labels: Any) -> Any:
        """(the shard's share of d_query, the dense gradient of its real rows)"""
        return nat.neg_score_shared_bwd_softmax(desc, query, self._candidates(shard, st.table),
                                                norm[:, 0].contiguous(), coef)

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
                raise RuntimeError(f"{type(self).__name__} runs eagerly: its step reads a flag on the host and cannot be "
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
        labels_all = self._query_labels(steps, rel_all)
        for shard, st, rows, relr, labels in zip(group.local_shards, steps, rows_all, rel_all, labels_all):
            dev = st.table.device
            idx = None
            if scheme == "h":  # gathered as [t, j, p] but wanted as [j, t, p]
                idx = self._static_map(
                    ("smT", n, st.ppp),
                    lambda: torch.arange(n * n * st.ppp).reshape(n, n, st.ppp).transpose(0, 1).reshape(-1), dev)
            ent = RowSource(rows.reshape(-1, W), idx)
            rel_q = relr.reshape(-1).contiguous()
            query, qctx = fn.query_fwd(side, ent, rel_q)
            state = self._shard_partial(shard, st, desc, query, labels)
            partials.append(state.reshape(n, n * st.ppp, -1))
            q_state.append((ent, rel_q, query, qctx, labels))
        ml_back = group.all_to_all(partials)  # [n(shard), S, 2] at the triples' owner
        tails_in = group.all_to_all(tails_out)
        outs, norms, coefs, rp_lse = [], [], [], []
        d_pos = -1.0
        for st, b, ml, tl in zip(steps, batches, ml_back, tails_in):
            dev = st.table.device
            st.recv = tl.reshape(-1, W)
            st.tail = RowSource(st.recv, None)
            st.positive_score, st.triple_ctx = fn.triple_fwd(RowSource(st.table, st.head_idx), st.tail, st.rel_idx)
            # the n partials of a query, merged in shard order
            norm, term, d_pos = self._merge_partials(ml, st.positive_score)
            w = self._triple_weight(b, dev, scale)
            coef = (w * float(self.loss_fn.loss_scale)).expand(term.shape[0]).contiguous()
            loss = (coef * term).sum().reshape(1)
            rp = None
            if self.relation_prediction_weight > 0.0:  # the relation of every triple against all relations
                rp_lse.append(nat.relation_lse_fwd(desc, RowSource(st.table, st.head_idx), st.tail,
                                                   fn.relation_embedding.data))
                rp = (coef * (rp_lse[-1] - st.positive_score)).sum().reshape(1)
                loss = loss + self.relation_prediction_weight * rp
            out: Dict[str, Any] = dict(loss=(loss if scale == 1.0 else loss / scale).reshape(()),
                                       positive_score=st.positive_score.to(fn.relation_embedding.dtype))
            if rp is not None:
                out["relation_prediction"] = (rp if scale == 1.0 else rp / scale).reshape(())
            outs.append(out)
            norms.append(norm)
            coefs.append(coef)
        return dict(steps=steps, q_state=q_state, outs=outs, norm=norms, coef=coefs, d_pos=d_pos, rp_lse=rp_lse)

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
        # positives: d loss / d pos = -coef (times the positive label's weight under KvsAll)
        d_tails = []
        for i, (sh, b, out, coef) in enumerate(zip(shards, batches, outs, fwd["coef"])):
            st = sh.step
            dh, dt = fn.triple_bwd(RowSource(st.table, st.head_idx), st.tail, st.rel_idx, st.triple_ctx,
                                   (fwd["d_pos"] * coef).contiguous(), d_rel)
            if self.relation_prediction_weight > 0.0:
                nat.relation_lse_bwd(desc, RowSource(st.table, st.head_idx), st.tail, fn.relation_embedding.data,
                                     st.rel_idx, fwd["rp_lse"][i], (self.relation_prediction_weight * coef).contiguous(),
                                     dh, dt, d_rel)
            if self.regularizer is not None:
                self._regularize(st, b, out, grad_scale, dh, dt, d_rel)
            sh.rows.append((st.head_idx, dh))
            d_tails.append(dt.reshape(n, st.ppp, W))
        d_tail_back = group.all_to_all(d_tails)
        # every shard needs (the rows' normalisers, coef) of the queries it scored
        norm_all = group.all_gather([torch.cat([z, c.reshape(-1, 1)], dim=1)
                                     for z, c in zip(fwd["norm"], fwd["coef"])])  # [n(j), S, m + 1]
        d_q = []
        for shard, sh, dtb, norm, (ent, rel_q, query, qctx, labels) in zip(group.local_shards, shards, d_tail_back,
                                                                          norm_all, fwd["q_state"]):
            st = sh.step
            dev = st.table.device
            sh.rows.append((st.local_tail.reshape(-1), dtb.reshape(-1, W)))
            norm = norm.reshape(-1, norm.shape[-1])
            dq, dn = self._shard_backward(shard, st, desc, query, norm[:, :-1], norm[:, -1].contiguous(), labels)
            rows = self._static_map(("1vsall rows", dn.shape[0]), lambda: torch.arange(dn.shape[0]), dev)
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
