"""KvsAll training: a binary cross entropy over EVERY entity of the graph, in which all *known* completions of a
triple's query are positive labels and every other entity is a negative (the training mode of ConvE and TuckER,
LibKGE's "KvsAll", PyKEEN's LCWA with BCE) - without the `[S, n_entity]` score matrix or its gradient.

For a micro-batch of S triples of a replica and corruption scheme "t" ("h" is the mirror image), with q_i the query
(h_i, r_i, ?), e running over every real entity of every shard, K_i the entities e != t_i with (h_i, r_i, e) in the
model's `KnownTripleFilter`, eps the label smoothing, smooth = eps / n_entity and pw = 1 - eps:

    A_i = sum_e softplus(s_ie)      B_i = sum_e s_ie      C_i = sum_{e in K_i} s_ie
    loss = sum_i coef_i * ( A_i - smooth * B_i - pw * (C_i + pos_i) ),    coef_i = loss_scale * w_i

which is sum_e BCEWithLogits(s_ie, pw * [e in K_i or e == t_i] + smooth): the true completion is labelled whether
or not the filter holds the triple.  `pos_i` is `score_triple`, w_i = triple_weight x triple_mask.

The data flow is `OneVsAllBessKGE`'s; what differs is what a shard computes for the queries of all replicas:

  labels    the local rows of the kept entity and of the true completion are all-gathered beside the relation ids;
            `KnownTripleFilter.completions` lists, on the device, every query's known completions that live on
            this shard (without the true one); `sharding.entity_to_idx` turns them into local rows - positions in
            the candidate list `table[:shard_counts[shard]]`.
  forward   `nat.neg_score_shared_bce` -> (A, B), `nat.label_score_sums` -> C: three floats per (query, shard) go
            to the owners and are summed in shard order.
  backward  coef is all-gathered; `nat.neg_score_shared_bwd_bce` gives the dense gradient of the shard's rows and its
            share of d_query; `triple_bwd` runs with d_pos = -pw * coef.
"""

import copy
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from besskge import _native as nat
from besskge.bess import _ReplicaStep
from besskge.loss import AllEntitiesBCELoss, BaseLossFunction
from besskge.negative_filter import KnownTripleFilter
from besskge.negative_sampler import ShardedNegativeSampler
from besskge.one_vs_all import OneVsAllBessKGE
from besskge.regularizer import EmbeddingRegularizer
from besskge.scoring import BaseScoreFunction

_Labels = Tuple[torch.Tensor, torch.Tensor]  # (ptr int64 [n_query + 1], positions in the shard's candidate list int32)


class KvsAllBessKGE(OneVsAllBessKGE):
    """Training step whose labels are all known completions, over all entities (see the module docstring).  Eager
    only: beside 1vsAll's flag the step reads the total of the label lists on the host."""

    def __init__(
        self,
        negative_sampler: ShardedNegativeSampler,
        score_fn: BaseScoreFunction,
        loss_fn: BaseLossFunction,
        known_triples: Union[KnownTripleFilter, Sequence[np.ndarray]],
        regularizer: Optional[EmbeddingRegularizer] = None,
        relation_prediction_weight: float = 0.0,
    ) -> None:
        """
        :param negative_sampler: `PlaceholderNegativeSampler("h" | "t")` (nothing is sampled).
        :param score_fn: TransE, RotatE, DistMult, ComplEx, TuckER, RESCAL, StructuredBilinear or ConvE (tails only).
        :param loss_fn: `AllEntitiesBCELoss(n_entity=sharding.n_entity, label_smoothing, loss_scale)`.
        :param known_triples: the triples whose completions are positive labels (usually the training set), global
            ids: a `KnownTripleFilter` or a list of [n, 3] arrays; built once, uploaded to each local device.
        :param regularizer: as for the other schemes.
        :param relation_prediction_weight: as for `OneVsAllBessKGE` (DistMult / ComplEx).
        """
        super().__init__(negative_sampler, score_fn, loss_fn, None, regularizer,
                         relation_prediction_weight=relation_prediction_weight)
        n_relation = int(score_fn.relation_embedding.shape[0])
        if not isinstance(known_triples, KnownTripleFilter):
            known_triples = KnownTripleFilter(known_triples, self.sharding.n_entity, n_relation)
        if known_triples.n_entity != self.sharding.n_entity or known_triples.n_relation_type != n_relation:
            raise ValueError(f"KvsAllBessKGE: the filter indexes {known_triples.n_entity} entities and "
                             f"{known_triples.n_relation_type} relation types, the model has "
                             f"{self.sharding.n_entity} and {n_relation}")
        self.known_triples = known_triples
        self._filters: Dict[torch.device, KnownTripleFilter] = {}
        self._label_maps: Dict[Any, torch.Tensor] = {}

    def _check_loss(self, loss_fn: BaseLossFunction, score_fn: BaseScoreFunction) -> None:
        if not isinstance(loss_fn, AllEntitiesBCELoss) or int(loss_fn.n_entity) != int(score_fn.sharding.n_entity):
            raise ValueError("KvsAllBessKGE: the loss is AllEntitiesBCELoss(n_entity=sharding.n_entity)")

    # ------------------------------------------------------------------ labels
    def _filter_on(self, dev: torch.device) -> KnownTripleFilter:
        if dev not in self._filters:
            f = self.known_triples
            self._filters[dev] = f if f.device == dev else copy.copy(f).to(dev)
        return self._filters[dev]

    def _entity_mask(self, shard: int, dev: torch.device) -> torch.Tensor:
        """uint8 [n_entity]: the entities whose rows this shard holds."""
        key = (shard, dev)
        if key not in self._label_maps:
            mask = torch.from_numpy((self.sharding.entity_to_shard == shard).astype(np.uint8))
            self._label_maps[key] = mask.to(dev).contiguous()
            torch.cuda.current_stream(dev).synchronize()
        return self._label_maps[key]

    def _query_labels(self, steps: List[_ReplicaStep], rel_all: List[torch.Tensor]) -> List[_Labels]:
        group = self._group()
        n = group.n_shard
        tail_side = self.negative_sampler.corruption_scheme == "t"
        heads_all = group.all_gather([st.sm_head for st in steps])  # [n(r), n(j), ppp]: rows of shard r
        tails_all = group.all_gather([st.local_tail for st in steps])  # [n(j), n(r), ppp]: rows of shard j
        sharding = self.sharding
        out = []
        for shard, st, heads, tails, relr in zip(group.local_shards, steps, heads_all, tails_all, rel_all):
            dev = st.table.device
            # queries in (owner r, tail shard j, q) order, as the query matrix
            owner = self._static_map(("kvsall owner", n, st.ppp),
                                     lambda: torch.arange(n).repeat_interleave(n * st.ppp), dev)
            other = self._static_map(("kvsall other", n, st.ppp),
                                     lambda: torch.arange(n).repeat_interleave(st.ppp).repeat(n), dev)
            l2g = self._static_map("kvsall l2g", lambda: torch.from_numpy(sharding.shard_and_idx_to_entity.astype(np.int64)),
                                   dev)
            e2i = self._static_map("kvsall e2i", lambda: torch.from_numpy(sharding.entity_to_idx.astype(np.int64)), dev)
            head_rows = heads.reshape(-1).contiguous()
            tail_rows = tails.transpose(0, 1).reshape(-1).contiguous()
            kept, kept_shard = (head_rows, owner) if tail_side else (tail_rows, other)
            true, true_shard = (tail_rows, other) if tail_side else (head_rows, owner)
            skip = l2g[true_shard.long(), true.long()].contiguous()
            ptr, ids = self._filter_on(dev).completions(kept, relr.reshape(-1).contiguous(), "t" if tail_side else "h",
                                                        skip=skip, keep_entity=self._entity_mask(shard, dev),
                                                        kept_shard=kept_shard, local_to_global=l2g)
            out.append((ptr, e2i[ids.long()].contiguous()))
        return out

    # ------------------------------------------------------- the loss' pieces
    def _shard_partial(self, shard: int, st: _ReplicaStep, desc: Any, query: torch.Tensor, labels: _Labels
                       ) -> torch.Tensor:
        cand = self._candidates(shard, st.table)
        ab = nat.neg_score_shared_bce(desc, query, cand)
        c = nat.label_score_sums(desc, query, cand, labels[0], labels[1], validate=False)
        return torch.cat([ab, c.reshape(-1, 1)], dim=1)

    def _merge_partials(self, part: torch.Tensor, pos: torch.Tensor) -> Any:
        total = part[0]
        for s in range(1, part.shape[0]):  # (shard order)
            total = total + part[s]
        loss_fn = self.loss_fn
        term = total[:, 0] - loss_fn.positive_weight * (total[:, 2] + pos)
        if loss_fn.smooth != 0.0:
            term = term - loss_fn.smooth * total[:, 1]
        return total[:, :0], term, -loss_fn.positive_weight  # (the backward needs nothing of a row but its coef)

    def _shard_backward(self, shard: int, st: _ReplicaStep, desc: Any, query: torch.Tensor, norm: torch.Tensor,
                        coef: torch.Tensor, labels: _Labels) -> Any:
        return nat.neg_score_shared_bwd_bce(desc, query, self._candidates(shard, st.table), self.loss_fn.smooth,
                                            self.loss_fn.positive_weight, labels[0], labels[1], coef, validate=False)
