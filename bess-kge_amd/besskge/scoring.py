"""Scoring functions TransE / RotatE / DistMult / ComplEx on HIP kernels.

Host-side mirror of the reference interface (`besskge/scoring.py:28-462,
746-946`): same class names, constructor signatures, attributes
(`negative_sample_sharing` stays a plain mutable attribute) and method
semantics

    score_triple(h [S,W], r_id [S], t [S,W])            -> [S]
    score_heads(H [B,N,W], r_id [S], t [S,W])           -> [S, B*N] | [S, N]
    score_tails(h [S,W], r_id [S], T [B,N,W])           -> [S, B*N] | [S, N]

but every score is computed by `libbesskge_hip.so`:

    score            K2+K3  bess_score_triple_fwd
    query transform  K2+K6  bess_query_fwd     (h+r | rot(h,r) | h*r | cmul(h,r) ...)
    shared negatives K4     bess_neg_score_shared_fwd
    per-triple       K5     bess_neg_score_pertriple_fwd

There is no torch/CPU implementation behind these methods: tensors must live on
a HIP device.  Results are fp32 (accumulation is fp32 also for fp16 tables).

PairRE, TripleRE, InterHT and TranS (reference
`scoring.py:465-743, 1418-1750`) share one kernel family: their score is
`-|| U * c1(e) + V * c2(e) + R ||_p` with per-query vectors U, V, R and the
(optionally normalised) parts c1, c2 of the candidate row (`csrc/affine.hip`).
The fused BESS step runs entirely in those kernels (query transform
`[U | V | R]`, negative scoring, positive score = tail-corruption score of the one
true tail, and all backwards); the public `score_*` methods express the S-row
query transform with torch ops so that they stay differentiable through autograd.

ConvE (`scoring.py:949-1146`) keeps its query network (batch-norm, conv,
linear: dense parameters) as torch modules on the device; what is scored
against the candidates is a plain dot product over `[embedding | tail bias]`
rows with the query `[net(h, r) | 1]`, i.e. the DistMult kernels.

BoxE (`scoring.py:1149-1415`): the relation-side preprocessing (width
normalisation, box size, tanh of the box) and the positive score are torch ops
over S rows; candidates are scored by the `csrc/boxe.hip` kernels.

HAKE (Zhang et al. 2020; not in the reference): the modulus + phase distance.
The query `[U | R | Q_p]` and the positive score are torch ops over S rows;
candidates are scored by the `csrc/hake.hip` kernels.
"""

import struct
from abc import ABC, abstractmethod
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import torch

from besskge import _native as nat
from besskge import ops
from besskge.embedding import (
    init_KGE_normal,
    init_KGE_uniform,
    init_uniform_norm,
    init_uniform_rotation,
    init_xavier_norm,
    initialize_entity_embedding,
    initialize_relation_embedding,
    refactor_embedding_sharding,
)
from besskge.sharding import Sharding

_Init = Union[torch.Tensor, List[Callable[..., torch.Tensor]]]


def _placement(kw: Optional[Dict[str, Any]]) -> Dict[str, Any]:
    """`device=`, `shards=`, `dtype=` of the scorer constructors (extension of the reference
    signatures, keyword only): allocate just the shard slices this process hosts
    (`[len(shards), M, W]`), directly on `device`, in `dtype` - so that a rank of a multi-GPU job
    never materialises the whole `[n_shard, M, W]` table on the host (BASELINE config 5: 128 GB
    per shard).  Defaults reproduce the reference: whole table, CPU, float32."""
    kw = dict(kw or {})
    out = dict(device=kw.pop("device", None), shards=kw.pop("shards", None), dtype=kw.pop("dtype", None))
    if kw:
        raise TypeError(f"unexpected keyword arguments {sorted(kw)}")
    return out


class BaseScoreFunction(torch.nn.Module, ABC):
    """Base class of all scoring functions."""

    #: score every query against the negatives of the whole micro-batch
    negative_sample_sharing: bool
    #: entity sharding
    sharding: Sharding
    #: entity table [n_shard, max_entity_per_shard, W]
    entity_embedding: torch.nn.Parameter
    #: relation table [n_relation, Wr]
    relation_embedding: torch.nn.Parameter

    #: kernel id of the scorer (include/besskge_hip.h BESS_TRANSE ...)
    _scorer_id: int = -1

    def kernel_desc(self) -> nat.ModelDesc:
        """Descriptor handed to the kernels (dtype follows the tables).  Built once per (dtype, widths, norm,
        switches) and handed out again: callers that set flags take a copy first (`nat.copy_desc`) - a training
        step asks for it five times."""
        rel, ent = self.relation_embedding, self.entity_embedding
        key = (rel.dtype, int(ent.shape[-1]), int(rel.shape[-1]), int(getattr(self, "scoring_norm", 0)),
               bool(getattr(self, "fp32_math", False)), getattr(self, "distance_route", "direct") == "gram")
        cached = self.__dict__.get("_kernel_desc_cache")
        if cached is not None and cached[0] == key:
            return cached[1]
        d = nat.ModelDesc()
        d.scorer = self._scorer_id
        d.norm_p = key[3]
        d.dtype = nat._dtype_code(rel)
        d.width = key[1]
        d.rel_width = key[2]
        if 0 <= self._scorer_id <= nat.COMPLEX and key[4]:
            d.reserved[0] = nat.FLAG_FP32_MATH
        if key[5]:
            d.reserved[0] |= nat.FLAG_GRAM_L2
        self.__dict__["_kernel_desc_cache"] = (key, d)
        return d

    #: TransE / RotatE with p = 1 on fp16 tables score shared negatives with packed-fp16 kernels that
    #: round the query to fp16 first (what the reference's fp16 mode does); True keeps the query in
    #: fp32 and uses the fp32 kernels
    fp32_math: bool = False

    def _table_dtype(self, x: torch.Tensor) -> torch.Tensor:
        dt = self.relation_embedding.dtype
        return x if x.dtype == dt else x.to(dt)

    # ---- hooks used by the fused BESS step (besskge.bess) -----------------------
    #: per-triple negatives of the own shard can use the segmented K9 reduction
    #: (gradient recomputed per reference from the query) instead of a [S*N, W] gradient
    supports_fused_segments = True
    #: the training forward can accumulate d loss / d query next to the scores
    #: (`bess_neg_score_pertriple_fwd_dq`)
    supports_fused_forward = True
    #: the score is bilinear in (query, candidate row): d score / d candidate = query, whatever the candidate
    #: (DistMult, ComplEx) - a backward that already has d_query never reads the candidate rows again
    bilinear_candidates = False
    #: query_fwd + triple_fwd, and their backwards, also exist as ONE launch each
    #: (`bess_query_triple_fwd / _bwd`: TransE / RotatE / DistMult / ComplEx)
    supports_fused_query_triple = True

    def query_triple_fwd(self, side: int, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor,
                         jobs: Any = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(query matrix of the side's negative-scoring problem, positive scores) of the same triples.  `jobs`: copy /
        fill jobs of the step's prologue that ride in the same launch (`nat.query_triple_fwd`)."""
        return nat.query_triple_fwd(self.kernel_desc(), side, head, tail, self.relation_embedding.data, rel_idx,
                                    jobs=jobs)

    def query_triple_bwd(self, side: int, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor,
                         d_pos: torch.Tensor, dq: torch.Tensor, d_rel: torch.Tensor
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
        """(d_head rows, d_tail rows) of positive score + query together; relation gradient added to `d_rel`."""
        return nat.query_triple_bwd(self.kernel_desc(), side, head, tail, self.relation_embedding.data, rel_idx,
                                    d_pos, dq, d_rel)

    def query_triple_bwd_parts(self, side: int, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor,
                               d_pos: torch.Tensor, dq_parts: torch.Tensor, dneg_parts: torch.Tensor, neg_idx: torch.Tensor,
                               rows_acc: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], d_rel: torch.Tensor) -> None:
        """`query_triple_bwd` with every gradient row ADDED into accumulators over the tables' row spaces (`rows_acc` =
        heads', tails', candidates'), fed by the partial sums of `nat.neg_score_shared_bwd_parts`."""
        nat.query_triple_bwd_parts(self.kernel_desc(), side, head, tail, self.relation_embedding.data, rel_idx, d_pos,
                                   dq_parts, dneg_parts, neg_idx, rows_acc, d_rel)

    def dense_parameters(self) -> List[torch.nn.Parameter]:
        """Parameters besides the two embedding tables (ConvE's network); replicated like the
        relation table.  Their gradients are collected by `query_bwd` / `triple_bwd` in
        `dense_grads` (parameter -> fp32 gradient) and consumed by the training step."""
        return []

    def _collect_dense(self, grads: Any) -> None:
        store = self.__dict__.setdefault("dense_grads", {})
        for p, g in zip(self.dense_parameters(), grads):
            if g is not None:
                store[p] = g.float() if p not in store else store[p] + g.float()

    def query_fwd(self, side: int, ent: nat.RowSource, rel_idx: torch.Tensor) -> Tuple[torch.Tensor, Any]:
        """Query matrix of a negative-scoring problem and the context its backward needs."""
        return nat.query_fwd(self.kernel_desc(), side, ent, self.relation_embedding.data, rel_idx), None

    def query_bwd(self, side: int, ent: nat.RowSource, rel_idx: torch.Tensor, ctx: Any, dq: torch.Tensor,
                  d_rel: torch.Tensor) -> torch.Tensor:
        """Gradient wrt the rows of `ent`; the relation-table gradient is added to `d_rel`."""
        return nat.query_bwd(self.kernel_desc(), side, ent, self.relation_embedding.data, rel_idx, dq, d_rel)

    def triple_fwd(self, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor) -> Tuple[torch.Tensor, Any]:
        """Positive scores [S] (+ backward context)."""
        return nat.score_triple_fwd(self.kernel_desc(), head, tail, self.relation_embedding.data, rel_idx), None

    def triple_bwd(self, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor, ctx: Any,
                   d_pos: torch.Tensor, d_rel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(d_head rows, d_tail rows); the relation-table gradient is added to `d_rel`."""
        return nat.score_triple_bwd(self.kernel_desc(), head, tail, self.relation_embedding.data, rel_idx, d_pos,
                                    d_rel)

    def score_triple(
        self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor
    ) -> torch.Tensor:
        """Score (h, r, t) triples.

        :param head_emb: [batch, W] head embeddings.
        :param relation_id: [batch] relation IDs.
        :param tail_emb: [batch, W] tail embeddings.
        :return: [batch] scores.
        """
        return ops.ScoreTriple.apply(
            self.kernel_desc(),
            self._table_dtype(head_emb),
            self.relation_embedding,
            relation_id,
            self._table_dtype(tail_emb),
        )

    def score_heads(
        self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor
    ) -> torch.Tensor:
        """Score candidate heads against fixed (r, t) queries.

        :param head_emb: [B, n_heads, W], B = 1 or batch.
        :param relation_id: [batch].
        :param tail_emb: [batch, W].
        :return: [batch, B * n_heads] with negative sample sharing, else
            [batch, n_heads].
        """
        return ops.ScoreNegatives.apply(
            self.kernel_desc(),
            nat.CORRUPT_HEAD,
            bool(self.negative_sample_sharing),
            self._table_dtype(tail_emb),
            self.relation_embedding,
            relation_id,
            self._table_dtype(head_emb),
        )

    def score_tails(
        self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor
    ) -> torch.Tensor:
        """Score candidate tails against fixed (h, r) queries.

        :param head_emb: [batch, W].
        :param relation_id: [batch].
        :param tail_emb: [B, n_tails, W], B = 1 or batch.
        :return: [batch, B * n_tails] with negative sample sharing, else
            [batch, n_tails].
        """
        return ops.ScoreNegatives.apply(
            self.kernel_desc(),
            nat.CORRUPT_TAIL,
            bool(self.negative_sample_sharing),
            self._table_dtype(head_emb),
            self.relation_embedding,
            relation_id,
            self._table_dtype(tail_emb),
        )

    def forward(
        self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor
    ) -> torch.Tensor:
        """Same as :meth:`score_triple`."""
        return self.score_triple(head_emb, relation_id, tail_emb)

    def update_sharding(self, new_sharding: Sharding) -> None:
        """Re-shard the entity table for a different :class:`Sharding`."""
        self.entity_embedding = refactor_embedding_sharding(
            entity_embedding=self.entity_embedding,
            old_sharding=self.sharding,
            new_sharding=new_sharding,
        )
        self.sharding = new_sharding

    def _allocate(
        self,
        sharding: Sharding,
        n_relation_type: int,
        inverse_relations: bool,
        entity_initializer: _Init,
        relation_initializer: _Init,
        entity_width: int,
        relation_width: int,
        what: str,
        placement: Optional[Dict[str, Any]] = None,
    ) -> None:
        self.sharding = sharding
        pl = _placement(placement)
        self.entity_embedding = initialize_entity_embedding(
            sharding, entity_initializer, [entity_width], **pl
        )
        self.relation_embedding = initialize_relation_embedding(
            n_relation_type, inverse_relations, relation_initializer, [relation_width],
            device=pl["device"], dtype=pl["dtype"]
        )
        assert (
            self.entity_embedding.shape[-1] == entity_width
            and self.relation_embedding.shape[-1] == relation_width
        ), what


class DistanceBasedScoreFunction(BaseScoreFunction, ABC):
    """Scorers of the form -||query - entity||_p."""

    #: norms the scorer's kernels implement; None = any integer p >= 1 (TransE, RotatE: p = 1 and p = 2 have their
    #: own instruction sequences, every other p goes through powf - reference scoring.py:174 takes any p)
    supported_norms: Optional[Tuple[int, ...]] = None

    def __init__(self, negative_sample_sharing: bool, scoring_norm: int) -> None:
        """
        :param negative_sample_sharing: see :class:`BaseScoreFunction`.
        :param scoring_norm: p of the p-norm.
        """
        super().__init__()
        if int(scoring_norm) != scoring_norm or scoring_norm < 1:
            raise ValueError(f"scoring_norm must be an integer p >= 1, got {scoring_norm!r}")
        if self.supported_norms is not None and scoring_norm not in self.supported_norms:
            raise ValueError(f"the HIP kernels of {type(self).__name__} implement scoring_norm in {self.supported_norms}")
        self.negative_sample_sharing = negative_sample_sharing
        self.scoring_norm = int(scoring_norm)

    def _set_distance_route(self, distance_route: str) -> None:
        """`distance_route` of TransE / RotatE: "direct" scores shared candidates with the tile kernels of the
        p-norms; "gram" (p = 2 only) permits ||q - e||^2 = ||q||^2 + ||e||^2 - 2 q.e through the split-fp16 matrix-core
        product wherever the bilinear scorers take it (`BESS_FLAG_GRAM_L2`: all-entities scores, ranks, pruned stores,
        log-sum-exp and the backward; not the BCE calls of KvsAll), close pairs recomputed directly in the forward.
        Parameters and state dicts are those of "direct"; the attribute can be reassigned."""
        if distance_route not in ("direct", "gram"):
            raise ValueError(f'{type(self).__name__}: distance_route is "direct" or "gram", got {distance_route!r}')
        if distance_route == "gram" and self.scoring_norm != 2:
            raise ValueError(f'{type(self).__name__}: distance_route="gram" is the Euclidean distance, scoring_norm=2')
        self.distance_route = distance_route

    def reduce_embedding(self, v: torch.Tensor) -> torch.Tensor:
        """p-norm over the embedding dimension (reference scoring.py:163-174)."""
        return torch.norm(v, p=self.scoring_norm, dim=-1)

    def broadcasted_distance(self, v1: torch.Tensor, v2: torch.Tensor) -> torch.Tensor:
        """Distances of queries v1 [batch, W] to candidates v2 [B, n_neg, W]: [batch, B * n_neg]
        with negative sample sharing, [batch, n_neg] otherwise (reference scoring.py:176-200);
        the HIP negative-scoring kernels with an identity query transform."""
        return -ops.ReduceNegatives.apply(_plain_desc(nat.TRANSE, self.scoring_norm, v2), bool(self.negative_sample_sharing),
                                          v1.float().contiguous(), v2)


def _plain_desc(scorer: int, norm_p: int, rows: torch.Tensor) -> nat.ModelDesc:
    """Descriptor of a bare reduction (`-||q - e||_p` or `<q, e>`) over rows of this dtype / width."""
    d = nat.ModelDesc()
    d.scorer, d.norm_p = scorer, int(norm_p)
    d.dtype = nat._dtype_code(rows)
    d.width = d.rel_width = int(rows.shape[-1])
    return d


class MatrixDecompositionScoreFunction(BaseScoreFunction, ABC):
    """Scorers of the form <query, entity>."""

    def __init__(self, negative_sample_sharing: bool) -> None:
        super().__init__()
        self.negative_sample_sharing = negative_sample_sharing

    def reduce_embedding(self, v: torch.Tensor) -> torch.Tensor:
        """Sum over the embedding dimension (reference scoring.py:219-229)."""
        return torch.sum(v, dim=-1)

    def broadcasted_dot_product(self, v1: torch.Tensor, v2: torch.Tensor) -> torch.Tensor:
        """Dot products of queries v1 [batch, W] with candidates v2 [B, n_neg, W]: [batch, B * n_neg]
        with negative sample sharing, [batch, n_neg] otherwise (reference scoring.py:231-255)."""
        return ops.ReduceNegatives.apply(_plain_desc(nat.DISTMULT, 0, v2), bool(self.negative_sample_sharing),
                                         v1.float().contiguous(), v2)


class TransE(DistanceBasedScoreFunction):
    """TransE: -|| h + r - t ||_p  (reference scoring.py:258-354)."""

    _scorer_id = nat.TRANSE

    def __init__(
        self,
        negative_sample_sharing: bool,
        scoring_norm: int,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        entity_initializer: _Init = [init_KGE_uniform],
        relation_initializer: _Init = [init_KGE_uniform],
        inverse_relations: bool = False,
        distance_route: str = "direct",
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing, scoring_norm)
        self._set_distance_route(distance_route)
        self._allocate(
            sharding, n_relation_type, inverse_relations, entity_initializer,
            relation_initializer, embedding_size, embedding_size,
            "TransE requires `embedding_size` embedding parameters"
            " for each entity and relation",
            placement=placement,
        )
        self.embedding_size = embedding_size


class RotatE(DistanceBasedScoreFunction):
    """RotatE: -|| h * e^{i r} - t ||_p over the [re | im] components
    (reference scoring.py:357-462; relation rows are phases)."""

    _scorer_id = nat.ROTATE

    def __init__(
        self,
        negative_sample_sharing: bool,
        scoring_norm: int,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        entity_initializer: _Init = [init_KGE_uniform],
        relation_initializer: _Init = [init_uniform_rotation],
        inverse_relations: bool = False,
        distance_route: str = "direct",
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing, scoring_norm)
        self._set_distance_route(distance_route)
        self._allocate(
            sharding, n_relation_type, inverse_relations, entity_initializer,
            relation_initializer, 2 * embedding_size, embedding_size,
            "RotatE requires `2*embedding_size` embedding parameters for each entity"
            " and `embedding_size` embedding parameters for each relation",
            placement=placement,
        )
        self.embedding_size = embedding_size


class DistMult(MatrixDecompositionScoreFunction):
    """DistMult: sum(h * r * t)  (reference scoring.py:746-837)."""

    _scorer_id = nat.DISTMULT
    bilinear_candidates = True

    def __init__(
        self,
        negative_sample_sharing: bool,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        entity_initializer: _Init = [init_KGE_uniform],
        relation_initializer: _Init = [init_KGE_uniform],
        inverse_relations: bool = False,
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing)
        self._allocate(
            sharding, n_relation_type, inverse_relations, entity_initializer,
            relation_initializer, embedding_size, embedding_size,
            "DistMult requires `embedding_size` embedding parameters"
            " for each entity and relation",
            placement=placement,
        )
        self.embedding_size = embedding_size


class ComplEx(MatrixDecompositionScoreFunction):
    """ComplEx: Re<h * r, conj t> on [re | im] rows (reference scoring.py:840-946)."""

    _scorer_id = nat.COMPLEX
    bilinear_candidates = True

    def __init__(
        self,
        negative_sample_sharing: bool,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        entity_initializer: _Init = [init_KGE_normal],
        relation_initializer: _Init = [init_KGE_normal],
        inverse_relations: bool = False,
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing)
        self._allocate(
            sharding, n_relation_type, inverse_relations, entity_initializer,
            relation_initializer, 2 * embedding_size, 2 * embedding_size,
            "ComplEx requires `2*embedding_size` embedding parameters"
            " for each entity and relation",
            placement=placement,
        )
        self.embedding_size = embedding_size


# --------------------------------------------------------------------------- #
# PairRE / TripleRE / InterHT / TranS: affine in the candidate
def _rows_of(src: nat.RowSource) -> torch.Tensor:
    return src.base if src.idx is None else nat.gather_rows(src.base, src.idx)


class _TorchQueryHooks:
    """Hooks of the fused step for scorers whose S-row work (query transform,
    positive score) is written with torch ops: autograd over S rows, the
    gradient of the embedding rows / relation table / dense parameters handed
    back to the step."""

    supports_fused_segments = False
    supports_fused_forward = False
    supports_fused_query_triple = False

    def _query_torch(self, side: int, rows: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def _triple_torch(self, h: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def query_fwd(self, side: int, ent: nat.RowSource, rel_idx: torch.Tensor) -> Tuple[torch.Tensor, Any]:
        track = torch.is_grad_enabled()  # inference runs under no_grad: no graph is kept
        rows = _rows_of(ent).detach().float().requires_grad_(track)
        rel = self.relation_embedding.detach().float().requires_grad_(track)  # type: ignore[attr-defined]
        q = self._query_torch(side, rows, rel, rel_idx)
        return q.detach().contiguous(), (rows, rel, q)

    def query_bwd(self, side: int, ent: nat.RowSource, rel_idx: torch.Tensor, ctx: Any, dq: torch.Tensor,
                  d_rel: torch.Tensor) -> torch.Tensor:
        rows, rel, q = ctx
        dense = self.dense_parameters()  # type: ignore[attr-defined]
        grads = torch.autograd.grad(q, [rows, rel] + dense, dq, allow_unused=True)
        d_rel += grads[1]
        self._collect_dense(grads[2:])  # type: ignore[attr-defined]
        return grads[0].contiguous()

    def triple_fwd(self, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor) -> Tuple[torch.Tensor, Any]:
        track = torch.is_grad_enabled()
        h = _rows_of(head).detach().float().requires_grad_(track)
        t = _rows_of(tail).detach().float().requires_grad_(track)
        rel = self.relation_embedding.detach().float().requires_grad_(track)  # type: ignore[attr-defined]
        sc = self._triple_torch(h, rel, rel_idx, t)
        return sc.detach().contiguous(), (h, t, rel, sc)

    def triple_bwd(self, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor, ctx: Any,
                   d_pos: torch.Tensor, d_rel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        h, t, rel, sc = ctx
        dense = self.dense_parameters()  # type: ignore[attr-defined]
        grads = torch.autograd.grad(sc, [h, t, rel] + dense, d_pos, allow_unused=True)
        d_rel += grads[2]
        self._collect_dense(grads[3:])  # type: ignore[attr-defined]
        return grads[0].contiguous(), grads[1].contiguous()


class _AffineScoreFunction(_TorchQueryHooks, DistanceBasedScoreFunction, ABC):
    """`-|| U * c1 + V * c2 + R ||_p` scorers; see the module docstring."""

    _scorer_id = nat.AFFINE
    supports_fused_segments = True  # csrc/affine.hip: k_aff_grad_segments
    #: d-wide parts of an entity row (1 | 2)
    _n_part: int = 1
    normalize: bool
    embedding_size: int

    #: member of the family as csrc/affine.hip numbers them (0 PairRE, 1 TripleRE, 2 InterHT, 3 TranS)
    _member: int = 0

    def _constant(self) -> float:
        """The model's additive constant (TripleRE: u, InterHT / TranS: offset)."""
        return 0.0

    def _host_constant(self, buf: torch.Tensor) -> float:
        """Value of a one-element constant buffer as a Python float, read from the device ONCE per version of the
        buffer: `float(device tensor)` is a host sync on every step - and an error inside a hipGraph capture
        (`tests/test_multi_gpu.py`, recorded TripleRE / InterHT / TranS steps)."""
        key = (buf.data_ptr(), buf._version, buf.device)
        cached = self.__dict__.get("_host_constant_cache")
        if cached is None or cached[0] != key:
            cached = (key, float(buf))
            self.__dict__["_host_constant_cache"] = cached
        return cached[1]

    def kernel_desc(self) -> nat.ModelDesc:
        d = super().kernel_desc()
        d.reserved[0] = self._n_part
        d.reserved[1] = int(bool(self.normalize)) | (self._member << 8)
        d.reserved[2] = struct.unpack("i", struct.pack("f", self._constant()))[0]
        return d

    # hooks of the fused step: HIP query transform (k_aff_query_fwd / bwd); the positive score is
    # the tail-corruption score of the one true tail (the same vector up to sign inside the norm)
    supports_fused_forward = False

    def query_fwd(self, side: int, ent: nat.RowSource, rel_idx: torch.Tensor) -> Tuple[torch.Tensor, Any]:
        return nat.query_fwd(self.kernel_desc(), side, ent, self.relation_embedding.data, rel_idx), None

    def query_bwd(self, side: int, ent: nat.RowSource, rel_idx: torch.Tensor, ctx: Any, dq: torch.Tensor,
                  d_rel: torch.Tensor) -> torch.Tensor:
        return nat.query_bwd(self.kernel_desc(), side, ent, self.relation_embedding.data, rel_idx, dq, d_rel)

    def triple_fwd(self, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor) -> Tuple[torch.Tensor, Any]:
        desc = self.kernel_desc()
        q = nat.query_fwd(desc, nat.CORRUPT_TAIL, head, self.relation_embedding.data, rel_idx)
        return nat.neg_score_pertriple_fwd(desc, q, tail, 1).reshape(-1), q

    def triple_bwd(self, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor, ctx: Any,
                   d_pos: torch.Tensor, d_rel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        desc = self.kernel_desc()
        dq, dt = nat.neg_score_pertriple_bwd(desc, ctx, tail, 1, d_pos.reshape(-1, 1).contiguous())
        dh = nat.query_bwd(desc, nat.CORRUPT_TAIL, head, self.relation_embedding.data, rel_idx, dq, d_rel)
        return dh, dt

    def _parts(self, x: torch.Tensor) -> List[torch.Tensor]:
        parts = list(torch.split(x.float(), self.embedding_size, dim=-1))
        if self.normalize:
            parts = [torch.nn.functional.normalize(p, p=2, dim=-1) for p in parts]
        return parts

    def _rel(self, relation_id: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
        return torch.index_select(table, 0, relation_id.reshape(-1).long()).float()

    @abstractmethod
    def _delta(self, h: List[torch.Tensor], rel: torch.Tensor, t: List[torch.Tensor]) -> torch.Tensor:
        """The vector whose p-norm is the (negated) score of a triple."""

    @abstractmethod
    def _uvr(self, side: int, kept: List[torch.Tensor], rel: torch.Tensor) -> List[torch.Tensor]:
        """[U, (V,) R] of the queries whose head (side = CORRUPT_HEAD) or tail is replaced."""

    def _score_norm(self, delta: torch.Tensor) -> torch.Tensor:
        return -torch.norm(delta, p=self.scoring_norm, dim=-1)

    # public API (differentiable through autograd + ops.ReduceNegatives)
    def score_triple(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_norm(self._delta(self._parts(head_emb), self._rel(relation_id, self.relation_embedding),
                                            self._parts(tail_emb)))

    def _score_candidates(self, side: int, kept: torch.Tensor, relation_id: torch.Tensor,
                          cand: torch.Tensor) -> torch.Tensor:
        q = torch.cat(self._uvr(side, self._parts(kept), self._rel(relation_id, self.relation_embedding)), dim=-1)
        return ops.ReduceNegatives.apply(self.kernel_desc(), bool(self.negative_sample_sharing), q.contiguous(),
                                         self._table_dtype(cand))

    def score_heads(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_HEAD, tail_emb, relation_id, head_emb)

    def score_tails(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_TAIL, head_emb, relation_id, tail_emb)

    def _query_torch(self, side: int, rows: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor) -> torch.Tensor:
        return torch.cat(self._uvr(side, self._parts(rows), self._rel(rel_idx, rel)), dim=-1)

    def _triple_torch(self, h: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        return self._score_norm(self._delta(self._parts(h), self._rel(rel_idx, rel), self._parts(t)))


class PairRE(_AffineScoreFunction):
    """PairRE: -|| h^ * r_h - t^ * r_t ||_p  (reference scoring.py:465-593)."""

    _n_part = 1
    _member = 0

    def __init__(
        self,
        negative_sample_sharing: bool,
        scoring_norm: int,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        entity_initializer: _Init = [init_KGE_uniform],
        relation_initializer: _Init = [init_KGE_uniform],
        normalize_entities: bool = True,
        inverse_relations: bool = False,
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing, scoring_norm)
        self.sharding = sharding
        self.normalize = normalize_entities
        if isinstance(relation_initializer, list):
            relation_initializer = 2 * relation_initializer
        self.entity_embedding = initialize_entity_embedding(sharding, entity_initializer, [embedding_size], **_placement(placement))
        # [r_h | r_t]: projections of heads and tails
        self.relation_embedding = initialize_relation_embedding(
            n_relation_type, inverse_relations, relation_initializer, [embedding_size, embedding_size],
            device=_placement(placement)["device"], dtype=_placement(placement)["dtype"])
        assert 2 * self.entity_embedding.shape[-1] == self.relation_embedding.shape[-1] == 2 * embedding_size, (
            "PairRE requires `embedding_size` embedding parameters for each entity"
            " and `2*embedding_size` embedding parameters for each relation")
        self.embedding_size = embedding_size

    def _delta(self, h: List[torch.Tensor], rel: torch.Tensor, t: List[torch.Tensor]) -> torch.Tensor:
        r_h, r_t = torch.split(rel, self.embedding_size, dim=-1)
        return h[0] * r_h - t[0] * r_t

    def _uvr(self, side: int, kept: List[torch.Tensor], rel: torch.Tensor) -> List[torch.Tensor]:
        r_h, r_t = torch.split(rel, self.embedding_size, dim=-1)
        if side == nat.CORRUPT_TAIL:  # t^ r_t - h^ r_h
            return [r_t, -(kept[0] * r_h)]
        return [r_h, -(kept[0] * r_t)]  # h^ r_h - t^ r_t


class TripleRE(_AffineScoreFunction):
    """TripleRE: -|| h^ * (r_h + u) - t^ * (r_t + u) + r_m ||_p  (reference scoring.py:596-743)."""

    _n_part = 1
    _member = 1

    def _constant(self) -> float:
        return self._host_constant(self.rel_u) if self.use_v2 else 0.0

    def __init__(
        self,
        negative_sample_sharing: bool,
        scoring_norm: int,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        entity_initializer: _Init = [init_KGE_uniform],
        relation_initializer: _Init = [init_KGE_uniform],
        normalize_entities: bool = True,
        u: float = 0.0,
        inverse_relations: bool = False,
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing, scoring_norm)
        self.sharding = sharding
        self.normalize = normalize_entities
        if isinstance(relation_initializer, list):
            relation_initializer = 3 * relation_initializer
        self.entity_embedding = initialize_entity_embedding(sharding, entity_initializer, [embedding_size], **_placement(placement))
        # [r_h | r_m | r_t]: head projection, translation, tail projection
        self.relation_embedding = initialize_relation_embedding(
            n_relation_type, inverse_relations, relation_initializer, [embedding_size] * 3,
            device=_placement(placement)["device"], dtype=_placement(placement)["dtype"])
        assert 3 * self.entity_embedding.shape[-1] == self.relation_embedding.shape[-1] == 3 * embedding_size, (
            "TripleRE requires `embedding_size` embedding parameters for each entity"
            " and `3*embedding_size` embedding parameters for each relation")
        self.embedding_size = embedding_size
        self.use_v2 = u > 0.0
        self.register_buffer("rel_u", torch.tensor([u], dtype=torch.float32))

    def _split(self, rel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        r_h, r_m, r_t = torch.split(rel, self.embedding_size, dim=-1)
        if self.use_v2:
            u = self.rel_u.to(rel.device)
            r_h, r_t = r_h + u, r_t + u
        return r_h, r_m, r_t

    def _delta(self, h: List[torch.Tensor], rel: torch.Tensor, t: List[torch.Tensor]) -> torch.Tensor:
        r_h, r_m, r_t = self._split(rel)
        return h[0] * r_h - t[0] * r_t + r_m

    def _uvr(self, side: int, kept: List[torch.Tensor], rel: torch.Tensor) -> List[torch.Tensor]:
        r_h, r_m, r_t = self._split(rel)
        if side == nat.CORRUPT_TAIL:  # t^ r_t - (h^ r_h + r_m)
            return [r_t, -(kept[0] * r_h + r_m)]
        return [r_h, -(kept[0] * r_t - r_m)]  # h^ r_h - (t^ r_t - r_m)


class InterHT(_AffineScoreFunction):
    """InterHT: -|| h^ * (t^_aux + o) + r - t^ * (h^_aux + o) ||_p  (reference scoring.py:1418-1572)."""

    _n_part = 2
    _member = 2

    def _constant(self) -> float:
        return self._host_constant(self.offset)

    def __init__(
        self,
        negative_sample_sharing: bool,
        scoring_norm: int,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        entity_initializer: _Init = [init_KGE_uniform],
        relation_initializer: _Init = [init_KGE_uniform],
        normalize_entities: bool = True,
        offset: float = 1.0,
        inverse_relations: bool = False,
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing, scoring_norm)
        self.sharding = sharding
        self.normalize = normalize_entities
        if isinstance(entity_initializer, list):
            entity_initializer = 2 * entity_initializer
        # [main | auxiliary]
        self.entity_embedding = initialize_entity_embedding(sharding, entity_initializer, [embedding_size] * 2, **_placement(placement))
        self.relation_embedding = initialize_relation_embedding(
            n_relation_type, inverse_relations, relation_initializer, [embedding_size],
            device=_placement(placement)["device"], dtype=_placement(placement)["dtype"])
        assert self.entity_embedding.shape[-1] == 2 * self.relation_embedding.shape[-1] == 2 * embedding_size, (
            "InterHT requires `2*embedding_size` embedding parameters for each entity"
            " and `embedding_size` embedding parameters for each relation")
        self.embedding_size = embedding_size
        self.register_buffer("offset", torch.tensor([offset], dtype=torch.float32))

    def _delta(self, h: List[torch.Tensor], rel: torch.Tensor, t: List[torch.Tensor]) -> torch.Tensor:
        o = self.offset.to(rel.device)
        return h[0] * (t[1] + o) + rel - t[0] * (h[1] + o)

    def _uvr(self, side: int, kept: List[torch.Tensor], rel: torch.Tensor) -> List[torch.Tensor]:
        o = self.offset.to(rel.device)
        main, aux = kept
        if side == nat.CORRUPT_TAIL:  # candidates t = (c1 main, c2 aux):  h_m (c2 + o) + r - c1 (h_a + o)
            return [-(aux + o), main, rel + main * o]
        return [aux + o, -main, rel - main * o]  # candidates h:  c1 (t_a + o) + r - t_m (c2 + o)


class TranS(_AffineScoreFunction):
    """TranS: -|| h^ * (t~ + o + r_bar) - t^ * (h~ + o - r_hat) + r ||_p  (reference scoring.py:1575-1750)."""

    _n_part = 2
    _member = 3

    def _constant(self) -> float:
        return self._host_constant(self.offset)

    def __init__(
        self,
        negative_sample_sharing: bool,
        scoring_norm: int,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        entity_initializer: _Init = [init_KGE_uniform],
        relation_initializer: _Init = [init_KGE_uniform],
        normalize_entities: bool = True,
        offset: float = 1.0,
        inverse_relations: bool = False,
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing, scoring_norm)
        self.sharding = sharding
        self.normalize = normalize_entities
        if isinstance(entity_initializer, list):
            entity_initializer = 2 * entity_initializer
        # [main | tilde]
        self.entity_embedding = initialize_entity_embedding(sharding, entity_initializer, [embedding_size] * 2, **_placement(placement))
        if isinstance(relation_initializer, list):
            relation_initializer = 3 * relation_initializer
        # [r | r_bar | r_hat]
        self.relation_embedding = initialize_relation_embedding(
            n_relation_type, inverse_relations, relation_initializer, [embedding_size] * 3,
            device=_placement(placement)["device"], dtype=_placement(placement)["dtype"])
        assert self.entity_embedding.shape[-1] / 2 == self.relation_embedding.shape[-1] / 3 == embedding_size, (
            "TranS requires `2*embedding_size` embedding parameters for each entity"
            " and `3*embedding_size` embedding parameters for each relation")
        self.embedding_size = embedding_size
        self.register_buffer("offset", torch.tensor([offset], dtype=torch.float32))

    def _delta(self, h: List[torch.Tensor], rel: torch.Tensor, t: List[torch.Tensor]) -> torch.Tensor:
        o = self.offset.to(rel.device)
        r, r_bar, r_hat = torch.split(rel, self.embedding_size, dim=-1)
        return h[0] * (t[1] + o + r_bar) - t[0] * (h[1] + o - r_hat) + r

    def _uvr(self, side: int, kept: List[torch.Tensor], rel: torch.Tensor) -> List[torch.Tensor]:
        o = self.offset.to(rel.device)
        r, r_bar, r_hat = torch.split(rel, self.embedding_size, dim=-1)
        main, tilde = kept
        if side == nat.CORRUPT_TAIL:  # h_m (c2 + o + r_bar) - c1 (h~ + o - r_hat) + r
            return [-(tilde + o - r_hat), main, r + main * (o + r_bar)]
        return [tilde + o + r_bar, -main, r - main * (o - r_hat)]  # c1 (t~ + o + r_bar) - t_m (c2 + o - r_hat) + r


class ConvE(_TorchQueryHooks, MatrixDecompositionScoreFunction):
    """ConvE: <net(h, r), t> + b_t, scores not passed through a sigmoid; only
    tails can be corrupted (reference scoring.py:949-1146).

    `query_route` chooses how the query network between the stacked image and the FC output is computed; both read
    the parameters and buffers of the same `conv_layers` / `fc_layers` modules, so state dicts, checkpoints,
    `dense_parameters()` and optimiser state are identical and a model can switch route (`fn.query_route = ...`):

    * `"torch"` (default): the `torch.nn.Sequential` modules as they are (MIOpen conv, batch-norm, rocBLAS linear);
      the `[S, F]` feature map (F = output_channels x output pixels) is written and kept for autograd.
    * `"fused"`: `ops.ConvEQuery` (csrc/conve.hip): conv, the output-channel batch-norm folded into a channel affine,
      ReLU, the feature-map dropout as a channel mask and the FC product in one pass on the matrix cores, forward and
      backward, without ever writing the feature map; training-mode batch statistics come from
      `ops.ConvEChannelStats`.  What is `[Cout]`-, `[S, d]`- or image-sized (input batch-norm and dropout, the fold,
      the running statistics, FC bias, the last batch-norm, dropout and ReLU) stays torch.  Train and eval mode, with
      and without `batch_normalization`, all three dropouts.  Under dropout the two routes draw different masks from
      the same generator state (the feature-map mask is drawn as `[S, Cout]`, not by `Dropout2d`), so they agree in
      distribution, not sample by sample.  Images beyond what the kernels keep in LDS (include/besskge_hip.h) are
      refused at construction."""

    _scorer_id = nat.DISTMULT  # candidates see a dot product over [embedding | bias] rows
    supports_fused_segments = True  # ... so their K9 is the dot-product segmented reduction

    def __init__(
        self,
        negative_sample_sharing: bool,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        embedding_height: int,
        embedding_width: int,
        entity_initializer: _Init = [init_xavier_norm, torch.nn.init.zeros_],
        relation_initializer: _Init = [init_xavier_norm],
        inverse_relations: bool = True,
        input_channels: int = 1,
        output_channels: int = 32,
        kernel_height: int = 3,
        kernel_width: int = 3,
        input_dropout: float = 0.2,
        feature_map_dropout: float = 0.2,
        hidden_dropout: float = 0.3,
        batch_normalization: bool = True,
        query_route: str = "torch",
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing)
        if query_route not in ("torch", "fused"):
            raise ValueError(f'ConvE: query_route is "torch" or "fused", got {query_route!r}')
        self.query_route = query_route
        self.sharding = sharding
        if input_channels * embedding_width * embedding_height != embedding_size:
            raise ValueError("`embedding_size` needs to be equal to"
                             " `input_channels * embedding_width * embedding_height`")
        # [embedding | tail bias]
        self.entity_embedding = initialize_entity_embedding(sharding, entity_initializer, [embedding_size, 1], **_placement(placement))
        self.relation_embedding = initialize_relation_embedding(
            n_relation_type, inverse_relations, relation_initializer, [embedding_size],
            device=_placement(placement)["device"], dtype=_placement(placement)["dtype"])
        assert self.entity_embedding.shape[-1] - 1 == self.relation_embedding.shape[-1] == embedding_size, (
            "ConvE requires `embedding_size + 1` embedding parameters for each entity"
            " and `embedding_size` embedding parameters for each relation")
        self.embedding_size = embedding_size
        self.inp_channels = input_channels
        self.emb_h = embedding_height
        self.emb_w = embedding_width
        conv_layers = [
            torch.nn.Dropout(input_dropout),
            torch.nn.Conv2d(in_channels=input_channels, out_channels=output_channels,
                            kernel_size=(kernel_height, kernel_width)),
            torch.nn.ReLU(),
            torch.nn.Dropout2d(feature_map_dropout),
        ]
        fc_layers = [
            torch.nn.Linear(output_channels * (2 * embedding_height - kernel_height + 1)
                            * (embedding_width - kernel_width + 1), embedding_size),
            torch.nn.Dropout(hidden_dropout),
            torch.nn.ReLU(),
        ]
        if batch_normalization:
            conv_layers.insert(0, torch.nn.BatchNorm2d(input_channels))
            conv_layers.insert(3, torch.nn.BatchNorm2d(output_channels))
            fc_layers.insert(2, torch.nn.BatchNorm1d(embedding_size))
        self.conv_layers = torch.nn.Sequential(*conv_layers)
        self.fc_layers = torch.nn.Sequential(*fc_layers)
        if query_route == "fused":  # (host arithmetic: raises beyond the LDS-resident image limit)
            nat.conve_supported([input_channels, 2 * embedding_height, embedding_width, output_channels, kernel_height,
                                 kernel_width], embedding_size)

    def kernel_desc(self) -> nat.ModelDesc:
        d = super().kernel_desc()
        d.rel_width = d.width  # the dot-product kernels only see [embedding | bias] rows
        return d

    def dense_parameters(self) -> List[torch.nn.Parameter]:
        return list(self.conv_layers.parameters()) + list(self.fc_layers.parameters())

    def _net(self, head: torch.Tensor, rel: torch.Tensor) -> torch.Tensor:
        shape = (-1, self.inp_channels, self.emb_h, self.emb_w)
        hr = torch.cat([head[..., :-1].reshape(shape), rel.reshape(shape)], dim=-2)
        if self.query_route == "fused":
            return self._net_fused(hr)
        return self.fc_layers(self.conv_layers(hr).flatten(start_dim=1))

    def _net_fused(self, x: torch.Tensor) -> torch.Tensor:
        """`fc_layers(conv_layers(x).flatten(1))` with everything between the conv's input and the FC product in
        `ops.ConvEQuery`; the modules are read, not called, from the conv on."""
        layers = list(self.conv_layers)
        at = next(i for i, m in enumerate(layers) if isinstance(m, torch.nn.Conv2d))
        for m in layers[:at]:  # input batch-norm and dropout
            x = m(x)
        conv, rest = layers[at], layers[at + 1:]
        norm = rest[0] if isinstance(rest[0], torch.nn.BatchNorm2d) else None
        drop = rest[-1]
        K, S = conv.weight, x.shape[0]
        if norm is None:
            a, b = torch.ones_like(conv.bias), conv.bias
        else:
            if norm.training or norm.running_mean is None:  # batch statistics of conv + bias (the bias cancels in z)
                mean, m2 = ops.ConvEChannelStats.apply(x, K)
                count = S * (x.shape[2] - K.shape[2] + 1) * (x.shape[3] - K.shape[3] + 1)
                var = m2 / count
                if norm.training and norm.running_mean is not None:
                    with torch.no_grad():
                        norm.num_batches_tracked += 1
                        f = norm.momentum if norm.momentum is not None else 1.0 / float(norm.num_batches_tracked)
                        norm.running_mean.mul_(1 - f).add_(f * (mean + conv.bias))
                        norm.running_var.mul_(1 - f).add_(f * m2 / max(count - 1, 1))
                shift = 0.0 * conv.bias - mean  # (the bias stays in the graph: a zero gradient, as on the torch route)
            else:
                var, shift = norm.running_var, conv.bias - norm.running_mean
            a = torch.rsqrt(var + norm.eps)
            if norm.weight is not None:
                a = a * norm.weight
            b = shift * a if norm.bias is None else shift * a + norm.bias
        mask = None
        if drop.training and drop.p > 0:  # Dropout2d: whole channels, kept ones scaled by 1 / (1 - p)
            mask = torch.nn.functional.dropout(torch.ones(S, K.shape[0], dtype=torch.float32, device=x.device), drop.p)
        fc = self.fc_layers[0]
        y = ops.ConvEQuery.apply(x, K, a, b, mask, fc.weight) + fc.bias
        for m in list(self.fc_layers)[1:]:
            y = m(y)
        return y

    def _query_torch(self, side: int, rows: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor) -> torch.Tensor:
        if side != nat.CORRUPT_TAIL:
            raise NotImplementedError("ConvE should not be used with head corruption")
        q = self._net(rows.float(), torch.index_select(rel, 0, rel_idx.reshape(-1).long()).float())
        return torch.cat([q, torch.ones_like(q[:, :1])], dim=-1)  # x 1 picks up the tail bias

    def _triple_torch(self, h: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        q = self._net(h.float(), torch.index_select(rel, 0, rel_idx.reshape(-1).long()).float())
        t = t.float()
        return torch.sum(q * t[..., :-1], dim=-1) + t[..., -1]

    def score_triple(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._triple_torch(head_emb, self.relation_embedding, relation_id, tail_emb)

    def score_heads(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError("ConvE should not be used with head corruption")

    def score_tails(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        q = self._query_torch(nat.CORRUPT_TAIL, head_emb, self.relation_embedding, relation_id)
        return ops.ReduceNegatives.apply(self.kernel_desc(), bool(self.negative_sample_sharing), q.contiguous(),
                                         self._table_dtype(tail_emb))


def init_core_uniform(core: torch.Tensor) -> torch.Tensor:
    """U(-1, 1): the initialisation of TuckER's core tensor in Balazevic et al. 2019."""
    return torch.nn.init.uniform_(core, -1.0, 1.0)


class TuckER(_TorchQueryHooks, MatrixDecompositionScoreFunction):
    """TuckER (Balazevic et al. 2019): `sum_{k,a,b} r_k h_a W[k, a, b] t_b` with a dense core tensor shared by all
    relations.  Entity rows are `entity_embedding_size` (de) wide, relation rows `relation_embedding_size` (dr).

    The core is the parameter `core [dr * de, de]`, fp32: row (k, a), column b hold W[k, a, b] (relation, head,
    tail) - the right operand of the product `q = (r (x) x) core` that `csrc/tucker.hip` runs on the matrix cores
    (`ops.TuckerQuery`) without forming `r @ W` per triple.  Against the candidates the score is the dot product
    `<q, e>`: the DistMult kernels, as for ConvE.  Both corruption sides are served (heads: the same kernels read the
    core with its two entity axes exchanged).

    The query chain is the paper's: batch-norm and dropout on the kept entity rows, the core product, batch-norm and
    dropout on the query.  The paper's third dropout acts on the mixed `[de, de]` matrix `r @ W` of every triple;
    that matrix is never formed here, so that dropout is left out.

    `query_route` chooses how the core product is computed; both give the same query up to fp32 rounding:

    * `"outer"` (default): `ops.TuckerQuery`, `2 S dr de^2` FLOP per product - every triple is treated as having its
      own relation vector.  Nothing is held besides the operands.  Choose it when relations outnumber the batch, or
      when dr is small (at dr = 30 it is the faster one whatever the relation count).
    * `"relation"`: the mixed matrices `M = relation_embedding @ core.view(dr, de * de)` of ALL relations are formed
      once per query (`torch.matmul`), then every row is multiplied by the matrix of its own relation
      (`ops.RelationQuery`, csrc/relation_query.hip): `2 n_rel dr de^2 + 2 S de^2` FLOP.  Choose it when the relation
      count is well below the batch size S and dr is large (the paper's de = dr = 200 with a few hundred relations).
      It holds two `[n_rel, de * de]` fp32 buffers (M and, in training, its gradient), and loses when relations
      outnumber the batch."""

    _scorer_id = nat.DISTMULT  # candidates see a dot product with the query
    supports_fused_segments = True  # ... so their K9 is the dot-product segmented reduction

    def __init__(
        self,
        negative_sample_sharing: bool,
        sharding: Sharding,
        n_relation_type: int,
        entity_embedding_size: int,
        relation_embedding_size: int,
        entity_initializer: _Init = [init_xavier_norm],
        relation_initializer: _Init = [init_xavier_norm],
        core_initializer: Callable[[torch.Tensor], torch.Tensor] = init_core_uniform,
        inverse_relations: bool = False,
        input_dropout: float = 0.0,
        hidden_dropout: float = 0.0,
        batch_normalization: bool = False,
        query_route: str = "outer",
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing)
        if query_route not in ("outer", "relation"):
            raise ValueError(f'TuckER: query_route is "outer" or "relation", got {query_route!r}')
        self.query_route = query_route
        self._allocate(
            sharding, n_relation_type, inverse_relations, entity_initializer,
            relation_initializer, entity_embedding_size, relation_embedding_size,
            "TuckER requires `entity_embedding_size` embedding parameters for each entity"
            " and `relation_embedding_size` for each relation",
            placement=placement,
        )
        de, dr = int(entity_embedding_size), int(relation_embedding_size)
        self.entity_embedding_size, self.relation_embedding_size = de, dr
        core = torch.empty((dr * de, de), dtype=torch.float32, device=_placement(placement)["device"])
        self.core = torch.nn.Parameter(core_initializer(core))
        norm = [torch.nn.BatchNorm1d(de)] if batch_normalization else []
        self.input_layers = torch.nn.Sequential(*norm, torch.nn.Dropout(input_dropout))
        norm = [torch.nn.BatchNorm1d(de)] if batch_normalization else []
        self.hidden_layers = torch.nn.Sequential(*norm, torch.nn.Dropout(hidden_dropout))

    def kernel_desc(self) -> nat.ModelDesc:
        d = super().kernel_desc()
        d.rel_width = d.width  # the dot-product kernels only see entity rows and queries
        return d

    def dense_parameters(self) -> List[torch.nn.Parameter]:
        return [self.core] + list(self.input_layers.parameters()) + list(self.hidden_layers.parameters())

    def _query_torch(self, side: int, rows: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor) -> torch.Tensor:
        x, swap = self.input_layers(rows.float()), side == nat.CORRUPT_HEAD
        if self.query_route == "relation":
            de = self.entity_embedding_size
            mixed = torch.matmul(rel.float(), self.core.view(self.relation_embedding_size, de * de))
            return self.hidden_layers(ops.RelationQuery.apply(x, mixed, rel_idx, swap))
        r = torch.index_select(rel, 0, rel_idx.reshape(-1).long()).float()
        q = ops.TuckerQuery.apply(x, r, self.core, swap)
        return self.hidden_layers(q)

    def _triple_torch(self, h: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        return torch.sum(self._query_torch(nat.CORRUPT_TAIL, h, rel, rel_idx) * t.float(), dim=-1)

    def score_triple(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._triple_torch(head_emb, self.relation_embedding, relation_id, tail_emb)

    def _score_candidates(self, side: int, kept: torch.Tensor, relation_id: torch.Tensor,
                          candidates: torch.Tensor) -> torch.Tensor:
        q = self._query_torch(side, kept, self.relation_embedding, relation_id)
        return ops.ReduceNegatives.apply(self.kernel_desc(), bool(self.negative_sample_sharing), q.contiguous(),
                                         self._table_dtype(candidates))

    def score_heads(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_HEAD, tail_emb, relation_id, head_emb)

    def score_tails(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_TAIL, head_emb, relation_id, tail_emb)


class RESCAL(_TorchQueryHooks, MatrixDecompositionScoreFunction):
    """RESCAL (Nickel et al. 2011): `h^T M_r t` with a full matrix per relation - the bilinear model that DistMult
    (diagonal M_r), ComplEx and TuckER (M_r mixed from a shared core) restrict.  Entity rows are `embedding_size` (de)
    wide; relation rows are de * de wide and hold M_r row-major, head axis first.

    The query `q = h^T M_r` (tails as candidates) or `M_r t` (heads) is the relation-grouped product of
    csrc/relation_query.hip on the relation table itself (`ops.RelationQuery`): the batch is grouped by relation and
    every group is multiplied by its one matrix on the matrix cores; no `[S, de, de]` gather of the table is made.
    Against the candidates the score is the dot product `<q, e>`: the DistMult kernels, as for ConvE and TuckER.
    The relation-table gradient is dense (`[n_relation, de * de]`, zero for relations a batch does not name)."""

    _scorer_id = nat.DISTMULT  # candidates see a dot product with the query
    supports_fused_segments = True  # ... so their K9 is the dot-product segmented reduction

    def __init__(
        self,
        negative_sample_sharing: bool,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        entity_initializer: _Init = [init_xavier_norm],
        relation_initializer: _Init = [init_xavier_norm],
        inverse_relations: bool = False,
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing)
        de = int(embedding_size)
        if de < 1 or de != embedding_size:
            raise ValueError(f"RESCAL: embedding_size is a positive integer, got {embedding_size!r}")
        self._allocate(
            sharding, n_relation_type, inverse_relations, entity_initializer,
            relation_initializer, de, de * de,
            "RESCAL requires `embedding_size` embedding parameters for each entity"
            " and `embedding_size ** 2` for each relation",
            placement=placement,
        )
        self.embedding_size = de

    def kernel_desc(self) -> nat.ModelDesc:
        d = super().kernel_desc()
        d.rel_width = d.width  # the dot-product kernels only see entity rows and queries
        return d

    def _query_torch(self, side: int, rows: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor) -> torch.Tensor:
        return ops.RelationQuery.apply(rows.float(), rel, rel_idx, side == nat.CORRUPT_HEAD)

    def _triple_torch(self, h: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        return torch.sum(self._query_torch(nat.CORRUPT_TAIL, h, rel, rel_idx) * t.float(), dim=-1)

    def score_triple(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._triple_torch(head_emb, self.relation_embedding, relation_id, tail_emb)

    def _score_candidates(self, side: int, kept: torch.Tensor, relation_id: torch.Tensor,
                          candidates: torch.Tensor) -> torch.Tensor:
        q = self._query_torch(side, kept, self.relation_embedding, relation_id)
        return ops.ReduceNegatives.apply(self.kernel_desc(), bool(self.negative_sample_sharing), q.contiguous(),
                                         self._table_dtype(candidates))

    def score_heads(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_HEAD, tail_emb, relation_id, head_emb)

    def score_tails(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_TAIL, head_emb, relation_id, tail_emb)


class BoxE(_TorchQueryHooks, DistanceBasedScoreFunction):
    """BoxE (reference scoring.py:1149-1415): entities are [base | bump]; the head is
    bumped by the tail's bump and vice versa, and each bumped point is scored by a
    piecewise distance to its relation box.

    `query_route` chooses who does the S-row work of a step (box normalisation, query, positive score and their
    backward); parameters and state dicts are the same and a model can switch route (`fn.query_route = ...`):
      "torch"   torch ops and autograd over gathered rows (the default);
      "native"  the kernels of csrc/boxe_query.hip (`nat.boxe_query_fwd / _bwd`): rows read through their index, no
                autograd graph over the batch, the relation gradient summed per relation without atomics (bitwise
                reproducible); the public `score_*` methods are differentiable through `ops.BoxEQuery`.  The
                kernels' widths are the candidate kernels': `embedding_size` <= 512, <= 128 when not a multiple
                of 4 - a wider one is refused here."""

    _scorer_id = nat.BOXE

    supports_fused_segments = True  # csrc/boxe.hip: k_box_grad_segments

    def __init__(
        self,
        negative_sample_sharing: bool,
        scoring_norm: int,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        entity_initializer: _Init = [torch.nn.init.uniform_],
        relation_initializer: _Init = [torch.nn.init.uniform_, init_uniform_norm],
        apply_tanh: bool = True,
        dist_func_per_dim: bool = True,
        eps: float = 1e-6,
        inverse_relations: bool = False,
        query_route: str = "torch",
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing, scoring_norm)
        if query_route not in ("torch", "native"):
            raise ValueError(f'BoxE: query_route is "torch" or "native", got {query_route!r}')
        if query_route == "native" and (embedding_size > 512 or (embedding_size % 4 != 0 and embedding_size > 128)):
            raise ValueError(f'BoxE: query_route="native" takes embedding_size <= 512 (<= 128 when not a multiple of 4),'
                             f" got {embedding_size}")
        self.query_route = query_route
        self.apply_tanh = apply_tanh
        self.dist_func_per_dim = dist_func_per_dim
        self.eps = eps
        self.sharding = sharding
        if isinstance(entity_initializer, list):
            entity_initializer = 2 * entity_initializer
        if isinstance(relation_initializer, list):
            relation_initializer = 4 * [relation_initializer[0]] + 2 * [relation_initializer[1]]
        # [base | bump]
        self.entity_embedding = initialize_entity_embedding(sharding, entity_initializer, [embedding_size] * 2, **_placement(placement))
        # [head centre | tail centre | head width | tail width | head size, tail size]
        self.relation_embedding = initialize_relation_embedding(
            n_relation_type, inverse_relations, relation_initializer, [embedding_size] * 4 + [1, 1],
            device=_placement(placement)["device"], dtype=_placement(placement)["dtype"])
        assert 2 * self.entity_embedding.shape[-1] == self.relation_embedding.shape[-1] - 2 == 4 * embedding_size, (
            "BoxE requires `2*embedding_size` embedding parameters for each entity"
            " and `4*embedding_size + 2` embedding parameters for each relation")
        self.embedding_size = embedding_size

    def kernel_desc(self) -> nat.ModelDesc:
        d = super().kernel_desc()
        d.reserved[0] = int(bool(self.apply_tanh)) | (int(bool(self.dist_func_per_dim)) << 1)
        return d

    def _boxes(self, rel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(centre, half width) [S, 2 (head box, tail box), d] after the reference's normalisation."""
        d = self.embedding_size
        center = rel[:, : 2 * d].reshape(-1, 2, d)
        width = rel[:, 2 * d: 4 * d].reshape(-1, 2, d).abs()
        size = rel[:, 4 * d:].reshape(-1, 2, 1)
        geo_mean = torch.exp(torch.mean(torch.log(torch.clamp(width, min=self.eps)), dim=-1, keepdim=True))
        width = width / torch.clamp(geo_mean, min=self.eps) * (1.0 + torch.nn.functional.elu(size))
        if self.apply_tanh:
            low = torch.tanh(center - 0.5 * width)
            up = torch.tanh(low + width)
            center, width = 0.5 * (low + up), up - low
        return center, 0.5 * width

    def _box_distance(self, point: torch.Tensor, center: torch.Tensor, half: torch.Tensor) -> torch.Tensor:
        """-(||f_head|| + ||f_tail||) for bumped points [..., 2, d]."""
        if self.apply_tanh:
            point = torch.tanh(point)
        dist = (point - center).abs()
        grow = 1.0 + 2.0 * half
        inside = dist <= half
        if not self.dist_func_per_dim:
            inside = inside.all(dim=-1, keepdim=True)
        f = torch.where(inside, dist / grow, dist * grow - half * (grow - 1.0 / grow))
        return -torch.norm(f, p=self.scoring_norm, dim=-1).sum(-1)

    def boxe_score(self, bumped_ht: torch.Tensor, center_ht: torch.Tensor, width_ht: torch.Tensor,
                   box_size: torch.Tensor) -> torch.Tensor:
        """BoxE score of bumped points [..., 2, d] against boxes given by raw centres, widths
        [..., 2, d] and sizes [..., 2], with broadcasting (reference scoring.py:1250-1340)."""
        rel = torch.cat([center_ht.flatten(start_dim=-2), width_ht.flatten(start_dim=-2), box_size], dim=-1)
        lead = rel.shape[:-1]
        center, half = self._boxes(rel.reshape(-1, rel.shape[-1]).float())
        return self._box_distance(bumped_ht.float(), center.reshape(*lead, 2, -1), half.reshape(*lead, 2, -1))

    @staticmethod
    def _wide(x: torch.Tensor) -> torch.Tensor:
        """fp32 for the arithmetic; a float64 operand (the tests' reference) stays as it is"""
        return x if x.dtype == torch.float64 else x.float()

    def _triple_torch(self, h: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        d = self.embedding_size
        center, half = self._boxes(self._wide(torch.index_select(rel, 0, rel_idx.reshape(-1).long())))
        # head box sees h_base + t_bump, tail box sees t_base + h_bump
        point = self._wide(h).reshape(-1, 2, d) + self._wide(t).reshape(-1, 2, d).flip(-2)
        return self._box_distance(point, center, half)

    def _query_torch(self, side: int, rows: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor) -> torch.Tensor:
        d = self.embedding_size
        center, half = self._boxes(self._wide(torch.index_select(rel, 0, rel_idx.reshape(-1).long())))
        kept = self._wide(rows).reshape(-1, 2, d)
        # candidate part 0 (base) is shifted by the kept bump, part 1 (bump) by the kept base; the
        # base of a candidate tail meets the tail box, the base of a candidate head the head box
        box = (1, 0) if side == nat.CORRUPT_TAIL else (0, 1)
        return torch.cat([kept[:, 1], center[:, box[0]], half[:, box[0]],
                          kept[:, 0], center[:, box[1]], half[:, box[1]]], dim=-1)

    # hooks of the fused step, route "native": the entry points of csrc/boxe_query.hip, no autograd graph over S rows
    def _rows(self, src: nat.RowSource) -> nat.RowSource:
        dt = self.relation_embedding.dtype
        return src if src.base.dtype == dt else nat.RowSource(src.base.to(dt), src.idx)

    def query_fwd(self, side: int, ent: nat.RowSource, rel_idx: torch.Tensor) -> Tuple[torch.Tensor, Any]:
        if self.query_route != "native":
            return super().query_fwd(side, ent, rel_idx)
        return nat.boxe_query_fwd(self.kernel_desc(), side, self.eps, self._rows(ent), self.relation_embedding.data,
                                  rel_idx)[0], None

    def query_bwd(self, side: int, ent: nat.RowSource, rel_idx: torch.Tensor, ctx: Any, dq: torch.Tensor,
                  d_rel: torch.Tensor) -> torch.Tensor:
        if self.query_route != "native":
            return super().query_bwd(side, ent, rel_idx, ctx, dq, d_rel)
        return nat.boxe_query_bwd(self.kernel_desc(), side, self.eps, self._rows(ent), self.relation_embedding.data,
                                  rel_idx, dq, d_rel)[0]

    def triple_fwd(self, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor) -> Tuple[torch.Tensor, Any]:
        if self.query_route != "native":
            return super().triple_fwd(head, tail, rel_idx)
        return nat.boxe_query_fwd(self.kernel_desc(), nat.CORRUPT_TAIL, self.eps, self._rows(head),
                                  self.relation_embedding.data, rel_idx, other=self._rows(tail), want_query=False)[1], None

    def triple_bwd(self, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor, ctx: Any,
                   d_pos: torch.Tensor, d_rel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.query_route != "native":
            return super().triple_bwd(head, tail, rel_idx, ctx, d_pos, d_rel)
        return nat.boxe_query_bwd(self.kernel_desc(), nat.CORRUPT_TAIL, self.eps, self._rows(head),
                                  self.relation_embedding.data, rel_idx, None, d_rel, other=self._rows(tail),
                                  d_pos=d_pos.reshape(-1).contiguous())

    def score_triple(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        if self.query_route == "native":
            return ops.BoxEQuery.apply(self.kernel_desc(), nat.CORRUPT_TAIL, self.eps, self._table_dtype(head_emb),
                                       self.relation_embedding, relation_id, self._table_dtype(tail_emb))
        return self._triple_torch(head_emb, self.relation_embedding, relation_id, tail_emb)

    def _score_candidates(self, side: int, kept: torch.Tensor, relation_id: torch.Tensor,
                          cand: torch.Tensor) -> torch.Tensor:
        if self.query_route == "native":
            q = ops.BoxEQuery.apply(self.kernel_desc(), side, self.eps, self._table_dtype(kept), self.relation_embedding,
                                    relation_id, None)
        else:
            q = self._query_torch(side, kept, self.relation_embedding, relation_id)
        return ops.ReduceNegatives.apply(self.kernel_desc(), bool(self.negative_sample_sharing), q.contiguous(),
                                         self._table_dtype(cand))

    def score_heads(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_HEAD, tail_emb, relation_id, head_emb)

    def score_tails(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_TAIL, head_emb, relation_id, tail_emb)


def init_hake_modulus(embedding_table: torch.Tensor) -> torch.Tensor:
    """Relation moduli of HAKE start at 1."""
    return torch.nn.init.ones_(embedding_table)


class HAKE(_TorchQueryHooks, DistanceBasedScoreFunction):
    """HAKE (Zhang et al. 2020): entities are [phase | modulus], relations [phase | modulus | bias];

        score = -( modulus_weight * || h_m * (|r_m| + b') - t_m * (1 - b') ||_2
                   + phase_weight * || sin(phase_scale * (h_p - t_p) / 2 + r_p / 2) ||_1 ),   b' = max(min(b, 1), -|r_m|)

    Candidates are scored by the kernels of csrc/hake.hip against the query matrix `[U | R | Q_p]`; the S-row work
    (the query and the positive score) is torch ops.  Both weights are fixed hyperparameters (buffers), not learned;
    `modulus_weight` >= 0 is folded into the query.  `fp32_math = True` scores shared candidates with the
    row-streaming kernels (one hardware sine per element) instead of the LDS tile kernel."""

    _scorer_id = nat.HAKE
    supports_fused_segments = True  # csrc/hake.hip: k_hake_grad_segments

    def __init__(
        self,
        negative_sample_sharing: bool,
        sharding: Sharding,
        n_relation_type: int,
        embedding_size: int,
        modulus_weight: float = 1.0,
        phase_weight: float = 0.5,
        phase_scale: float = 1.0,
        entity_initializer: _Init = [init_uniform_rotation, init_KGE_uniform],
        relation_initializer: _Init = [init_uniform_rotation, init_hake_modulus, torch.nn.init.zeros_],
        inverse_relations: bool = False,
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing, 2)
        if modulus_weight < 0:
            raise ValueError(f"HAKE: modulus_weight must be >= 0 (it is folded into the query), got {modulus_weight!r}")
        limit = 512 if embedding_size % 4 == 0 else (256 if embedding_size % 2 == 0 else 128)
        if embedding_size > limit:
            raise ValueError(f"HAKE: the row kernels take embedding_size <= 512 (<= 256 when not a multiple of 4, <= 128 "
                             f"when odd), got {embedding_size}")
        self.sharding = sharding
        pl = _placement(placement)
        # [phase | modulus]
        self.entity_embedding = initialize_entity_embedding(sharding, entity_initializer, [embedding_size] * 2, **pl)
        # [phase | modulus | bias]
        self.relation_embedding = initialize_relation_embedding(
            n_relation_type, inverse_relations, relation_initializer, [embedding_size] * 3,
            device=pl["device"], dtype=pl["dtype"])
        assert 3 * self.entity_embedding.shape[-1] == 2 * self.relation_embedding.shape[-1] == 6 * embedding_size, (
            "HAKE requires `2*embedding_size` embedding parameters for each entity"
            " and `3*embedding_size` embedding parameters for each relation")
        self.embedding_size = embedding_size
        for name, value in (("modulus_weight", modulus_weight), ("phase_weight", phase_weight), ("phase_scale", phase_scale)):
            self.register_buffer(name, torch.tensor(float(value), dtype=torch.float32))

    @property
    def _weights(self) -> Tuple[float, float, float]:
        """(modulus_weight, phase_weight, phase_scale) as Python floats, read from the buffers ONCE per version of
        them (a loaded state dict changes them): `float(device tensor)` is a host sync on every step, and an error
        inside a hipGraph capture."""
        bufs = (self.modulus_weight, self.phase_weight, self.phase_scale)
        key = tuple((b.data_ptr(), b._version, b.device) for b in bufs)
        cached = self.__dict__.get("_weights_cache")
        if cached is None or cached[0] != key:
            cached = (key, tuple(float(b) for b in bufs))
            self.__dict__["_weights_cache"] = cached
        return cached[1]

    def kernel_desc(self) -> nat.ModelDesc:
        d = super().kernel_desc()
        d.reserved[0] = nat.FLAG_FP32_MATH if self.fp32_math else 0
        d.reserved[1] = struct.unpack("i", struct.pack("f", self._weights[1]))[0]
        d.reserved[2] = struct.unpack("i", struct.pack("f", self._weights[2]))[0]
        return d

    def _relation_parts(self, rel: torch.Tensor, rel_idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(r_p, |r_m| + b', 1 - b') of the triples' relations [S, d]"""
        r = BoxE._wide(torch.index_select(rel, 0, rel_idx.reshape(-1).long()))
        r_p, r_m, b = torch.split(r, self.embedding_size, dim=-1)
        r_m = r_m.abs()
        b = torch.maximum(torch.clamp(b, max=1.0), -r_m)
        return r_p, r_m + b, 1.0 - b

    def _triple_torch(self, h: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        lm, lp, ps = self._weights
        r_p, scale_h, scale_t = self._relation_parts(rel, rel_idx)
        h_p, h_m = torch.split(BoxE._wide(h), self.embedding_size, dim=-1)
        t_p, t_m = torch.split(BoxE._wide(t), self.embedding_size, dim=-1)
        modulus = torch.norm(h_m * scale_h - t_m * scale_t, p=2, dim=-1)
        phase = torch.sin((ps * (h_p - t_p) + r_p) / 2).abs().sum(-1)
        return -(lm * modulus + lp * phase)

    def _query_torch(self, side: int, rows: torch.Tensor, rel: torch.Tensor, rel_idx: torch.Tensor) -> torch.Tensor:
        lm, _, ps = self._weights
        r_p, scale_h, scale_t = self._relation_parts(rel, rel_idx)
        k_p, k_m = torch.split(BoxE._wide(rows), self.embedding_size, dim=-1)
        if side == nat.CORRUPT_TAIL:  # modulus difference U * t_m + R, phase difference Q_p - phase_scale * t_p
            return torch.cat([-lm * scale_t, lm * k_m * scale_h, ps * k_p + r_p], dim=-1)
        # the norm and |sin| are even: the head's modulus difference is taken as U * h_m + R with R = -t_m (1 - b'),
        # its phase difference as (phase_scale * t_p - r_p) - phase_scale * h_p
        return torch.cat([lm * scale_h, -lm * k_m * scale_t, ps * k_p - r_p], dim=-1)

    def score_triple(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._triple_torch(head_emb, self.relation_embedding, relation_id, tail_emb).float()

    def _score_candidates(self, side: int, kept: torch.Tensor, relation_id: torch.Tensor,
                          cand: torch.Tensor) -> torch.Tensor:
        q = self._query_torch(side, kept, self.relation_embedding, relation_id).float()
        return ops.ReduceNegatives.apply(self.kernel_desc(), bool(self.negative_sample_sharing), q.contiguous(),
                                         self._table_dtype(cand))

    def score_heads(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_HEAD, tail_emb, relation_id, head_emb)

    def score_tails(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_TAIL, head_emb, relation_id, tail_emb)


# --------------------------------------------------------------------------- #
# structured bilinear scorers: QuatE, SimplE, CP, ANALOGY, AutoSF from one term table
_Term = Tuple[int, int, int, float]


class StructuredBilinear(MatrixDecompositionScoreFunction):
    """`score(h, r, t) = sum over terms (i, j, k, c) of c * sum_x h[i d + x] r[j d + x] t[k d + x]`: entity rows are
    `n_entity_blocks` (K) blocks of `block_size` (d) columns, relation rows `n_relation_blocks` (Kr) blocks.
    DistMult is K = 1 with one term, ComplEx K = 2 with four, QuatE K = 4 with the 16 of the Hamilton product; an
    AutoSF result is such a list (`from_autosf`); `QuatE`, `SimplE`, `CP` and `ANALOGY` below fill in their tables.

    The score is bilinear in the candidate: the query `[term][column]` transform and its backward are the kernels of
    csrc/struct_query.hip (`nat.struct_query_fwd / _bwd`, no autograd graph over the batch, the relation gradient
    summed per relation without atomics: bitwise reproducible), and every candidate-side path is DistMult's.
    `relation_unit_norm`: every relation column is divided by its norm over the Kr blocks before use (QuatE's unit
    quaternion); the backward differentiates through it."""

    _scorer_id = nat.DISTMULT  # candidates see a dot product with the query
    bilinear_candidates = True
    supports_fused_segments = True
    supports_fused_forward = False
    supports_fused_query_triple = False

    def __init__(
        self,
        negative_sample_sharing: bool,
        sharding: Sharding,
        n_relation_type: int,
        block_size: int,
        terms: List[_Term],
        n_entity_blocks: int,
        n_relation_blocks: int,
        entity_initializer: _Init = [init_KGE_normal],
        relation_initializer: _Init = [init_KGE_normal],
        inverse_relations: bool = False,
        relation_unit_norm: bool = False,
        **placement: Any,
    ) -> None:
        super().__init__(negative_sample_sharing)
        K, Kr, d = int(n_entity_blocks), int(n_relation_blocks), int(block_size)
        if not (1 <= K <= nat.STRUCT_MAX_BLOCKS and 1 <= Kr <= nat.STRUCT_MAX_BLOCKS and d >= 1):
            raise ValueError(f"StructuredBilinear: 1 to {nat.STRUCT_MAX_BLOCKS} entity and relation blocks of at least one "
                             f"column, got {n_entity_blocks}, {n_relation_blocks} blocks of {block_size}")
        terms = [(int(i), int(j), int(k), float(c)) for i, j, k, c in terms]
        if not 1 <= len(terms) <= nat.STRUCT_MAX_TERMS:
            raise ValueError(f"StructuredBilinear: 1 to {nat.STRUCT_MAX_TERMS} terms, got {len(terms)}")
        for i, j, k, c in terms:
            if not (0 <= i < K and 0 <= j < Kr and 0 <= k < K):
                raise ValueError(f"StructuredBilinear: term {(i, j, k)} names a block outside ({K}, {Kr}, {K})")
            if c != c or c in (float("inf"), float("-inf")):
                raise ValueError(f"StructuredBilinear: the coefficient of term {(i, j, k)} is not finite")
        if len({t[:3] for t in terms}) != len(terms):
            raise ValueError("StructuredBilinear: a block triple (i, j, k) is named twice")
        self.terms, self.n_entity_blocks, self.n_relation_blocks, self.block_size = terms, K, Kr, d
        self.relation_unit_norm = bool(relation_unit_norm)
        self._allocate(
            sharding, n_relation_type, inverse_relations, entity_initializer, relation_initializer, K * d, Kr * d,
            "StructuredBilinear requires `n_entity_blocks * block_size` embedding parameters for each entity"
            " and `n_relation_blocks * block_size` for each relation",
            placement=placement,
        )

    @classmethod
    def from_autosf(cls, negative_sample_sharing: bool, sharding: Sharding, n_relation_type: int, block_size: int,
                    blocks: List[List[int]], **kwargs: Any) -> "StructuredBilinear":
        """The scoring function AutoSF prints as a K x K signed block matrix: entry (i, k) = +-(j + 1) puts relation
        block j between head block i and tail block k with that sign, 0 is no term."""
        K = len(blocks)
        if K < 1 or any(len(row) != K for row in blocks):
            raise ValueError("StructuredBilinear.from_autosf: a square matrix of signed relation block numbers")
        terms = [(i, abs(int(v)) - 1, k, 1.0 if v > 0 else -1.0) for i, row in enumerate(blocks)
                 for k, v in enumerate(row) if v]
        if any(t[1] >= K for t in terms):
            raise ValueError(f"StructuredBilinear.from_autosf: entries are 0 or +-1 .. +-{K}")
        return cls(negative_sample_sharing, sharding, n_relation_type, block_size, terms, K, K, **kwargs)

    def kernel_desc(self) -> nat.ModelDesc:
        d = super().kernel_desc()
        d.rel_width = d.width  # the dot-product kernels only see entity rows and queries
        return d

    def struct_desc(self) -> nat.StructDesc:
        """Descriptor of the term table for the tables' current type (built once per type)."""
        key = self.relation_embedding.dtype
        cached = self.__dict__.get("_struct_desc_cache")
        if cached is None or cached[0] != key:
            cached = (key, nat.struct_desc(self.relation_embedding, self.n_entity_blocks, self.n_relation_blocks,
                                           self.block_size, self.terms, self.relation_unit_norm))
            self.__dict__["_struct_desc_cache"] = cached
        return cached[1]

    # hooks of the fused step: the native entry points, no autograd graph over S rows
    def query_fwd(self, side: int, ent: nat.RowSource, rel_idx: torch.Tensor) -> Tuple[torch.Tensor, Any]:
        return nat.struct_query_fwd(self.struct_desc(), side, ent, self.relation_embedding.data, rel_idx)[0], None

    def query_bwd(self, side: int, ent: nat.RowSource, rel_idx: torch.Tensor, ctx: Any, dq: torch.Tensor,
                  d_rel: torch.Tensor) -> torch.Tensor:
        return nat.struct_query_bwd(self.struct_desc(), side, ent, self.relation_embedding.data, rel_idx, dq, d_rel)[0]

    def triple_fwd(self, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor) -> Tuple[torch.Tensor, Any]:
        return nat.struct_query_fwd(self.struct_desc(), nat.CORRUPT_TAIL, head, self.relation_embedding.data, rel_idx,
                                    other=tail)[1], None

    def triple_bwd(self, head: nat.RowSource, tail: nat.RowSource, rel_idx: torch.Tensor, ctx: Any,
                   d_pos: torch.Tensor, d_rel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return nat.struct_query_bwd(self.struct_desc(), nat.CORRUPT_TAIL, head, self.relation_embedding.data, rel_idx,
                                    None, d_rel, other=tail, d_pos=d_pos.reshape(-1).contiguous())

    # public API (differentiable: ops.StructuredQuery + ops.ReduceNegatives)
    def _query(self, side: int, kept: torch.Tensor, relation_id: torch.Tensor) -> torch.Tensor:
        return ops.StructuredQuery.apply(self.struct_desc(), side, self._table_dtype(kept), self.relation_embedding,
                                         relation_id)

    def score_triple(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return torch.sum(self._query(nat.CORRUPT_TAIL, head_emb, relation_id) * tail_emb.float(), dim=-1)

    def _score_candidates(self, side: int, kept: torch.Tensor, relation_id: torch.Tensor,
                          candidates: torch.Tensor) -> torch.Tensor:
        return ops.ReduceNegatives.apply(self.kernel_desc(), bool(self.negative_sample_sharing),
                                         self._query(side, kept, relation_id), self._table_dtype(candidates))

    def score_heads(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_HEAD, tail_emb, relation_id, head_emb)

    def score_tails(self, head_emb: torch.Tensor, relation_id: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        return self._score_candidates(nat.CORRUPT_TAIL, head_emb, relation_id, tail_emb)


#: h_i r_j enters component k of the Hamilton product h (x) r with this sign; the score is <h (x) r, t>
QUATE_TERMS: List[_Term] = [
    (0, 0, 0, 1.0), (0, 1, 1, 1.0), (0, 2, 2, 1.0), (0, 3, 3, 1.0),
    (1, 0, 1, 1.0), (1, 1, 0, -1.0), (1, 2, 3, 1.0), (1, 3, 2, -1.0),
    (2, 0, 2, 1.0), (2, 1, 3, -1.0), (2, 2, 0, -1.0), (2, 3, 1, 1.0),
    (3, 0, 3, 1.0), (3, 1, 2, 1.0), (3, 2, 1, -1.0), (3, 3, 0, -1.0)]
DISTMULT_TERMS: List[_Term] = [(0, 0, 0, 1.0)]
#: Re<h r, conj t> on [re | im] rows
COMPLEX_TERMS: List[_Term] = [(0, 0, 0, 1.0), (1, 1, 0, -1.0), (0, 1, 1, 1.0), (1, 0, 1, 1.0)]


def QuatE(negative_sample_sharing: bool, sharding: Sharding, n_relation_type: int, embedding_size: int,
          relation_unit_norm: bool = True, **kwargs: Any) -> StructuredBilinear:
    """QuatE (Zhang et al. 2019): `<h (x) r / |r|, t>` on quaternion rows `[a | b | c | d]` of 4 * embedding_size."""
    return StructuredBilinear(negative_sample_sharing, sharding, n_relation_type, embedding_size, QUATE_TERMS, 4, 4,
                              relation_unit_norm=relation_unit_norm, **kwargs)


def SimplE(negative_sample_sharing: bool, sharding: Sharding, n_relation_type: int, embedding_size: int,
           **kwargs: Any) -> StructuredBilinear:
    """SimplE (Kazemi & Poole 2018): entity rows `[head role | tail role]`, relation rows `[r | r_inv]`, the average of
    `<h_head, r, t_tail>` and `<t_head, r_inv, h_tail>`."""
    return StructuredBilinear(negative_sample_sharing, sharding, n_relation_type, embedding_size,
                              [(0, 0, 1, 0.5), (1, 1, 0, 0.5)], 2, 2, **kwargs)


def CP(negative_sample_sharing: bool, sharding: Sharding, n_relation_type: int, embedding_size: int,
       **kwargs: Any) -> StructuredBilinear:
    """Canonical polyadic decomposition: `<h_head, r, t_tail>` on role-split entity rows `[head role | tail role]`."""
    return StructuredBilinear(negative_sample_sharing, sharding, n_relation_type, embedding_size, [(0, 0, 1, 1.0)], 2, 1,
                              **kwargs)


def ANALOGY(negative_sample_sharing: bool, sharding: Sharding, n_relation_type: int, embedding_size: int,
            scalar_share: float = 0.5, **kwargs: Any) -> StructuredBilinear:
    """ANALOGY (Liu et al. 2017): a DistMult part and a ComplEx part side by side.  Rows are four blocks
    `[scalar | scalar | re | im]` of `embedding_size // 4` columns: `scalar_share` = 0.5 (two scalar blocks) is the
    paper's half-and-half split, 0 leaves ComplEx and 1 DistMult on blocks of `embedding_size // 2` and
    `embedding_size` columns."""
    if scalar_share == 0.5 and embedding_size % 4 == 0:
        return StructuredBilinear(negative_sample_sharing, sharding, n_relation_type, embedding_size // 4,
                                  [(0, 0, 0, 1.0), (1, 1, 1, 1.0)] + [(i + 2, j + 2, k + 2, c) for i, j, k, c in COMPLEX_TERMS],
                                  4, 4, **kwargs)
    if scalar_share == 0.0 and embedding_size % 2 == 0:
        return StructuredBilinear(negative_sample_sharing, sharding, n_relation_type, embedding_size // 2, COMPLEX_TERMS,
                                  2, 2, **kwargs)
    if scalar_share == 1.0:
        return StructuredBilinear(negative_sample_sharing, sharding, n_relation_type, embedding_size, DISTMULT_TERMS, 1, 1,
                                  **kwargs)
    raise ValueError("ANALOGY: scalar_share is 0, 0.5 (embedding_size a multiple of 4) or 1")
