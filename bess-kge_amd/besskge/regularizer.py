"""Embedding regulariser of the training step: Lp / N3 penalty on the rows of the positive triples.

The reference has no regulariser; the literature's ComplEx / DistMult results are ComplEx-N3 / DistMult-N3 (Lacroix,
Usunier, Obozinski 2018, "Canonical tensor decomposition for knowledge base completion"; LibKGE; DGL-KE `-rc / -rn 3`).
One HIP launch behind the step's backward (`bess_regularize_triples`) adds the penalty's gradient to the gradient
rows the backward kernels have left, so no update list, optimiser or scoring kernel knows about it.
"""

import math
from typing import Any, Optional, Tuple

from besskge import _native as nat


class EmbeddingRegularizer:
    """Penalty on the embeddings of a micro-batch's positive triples (h_i, r_i, t_i), added to the loss:

        R = sum_i c_i * ( entity_coef * (Phi(h_i) + Phi(t_i)) + relation_coef * Phi(r_i) ),   Phi(x) = sum_k |x_k|^p

    with c_i = loss_scale * triple_weight_i, the factor the loss gives triple i (so R is scaled with the loss, under
    gradient accumulation too).  With `complex_modulus` the rows are [re(d) | im(d)] and Phi(x) = sum_k
    (re_k^2 + im_k^2)^(p/2): p = 3 is the nuclear 3-norm "N3" of Lacroix et al.

    This is Lacroix's per-triple ("weighted") form: an entity or relation is penalised once per occurrence in a
    positive triple of the micro-batch, i.e. in proportion to its frequency.  Only the positives are penalised: the
    rows of the negative samples get no penalty, whatever the corruption scheme.

    It is not `weight_decay` of the `besskge.runtime` optimisers: that is plain L2 (p = 2 on coordinates), decays a row
    once per optimiser step in which the row is touched - negatives included, however often it occurs - is not part
    of the reported loss and is applied inside the optimiser (decoupled from the loss's scale and weights).

    :param p: exponent, any real p >= 1 (2 and 3 take no `powf`).
    :param entity_coef: coefficient of head and tail rows, >= 0.
    :param relation_coef: coefficient of relation rows; None: as `entity_coef`.
    :param complex_modulus: penalise complex moduli.  None: where the scorer's rows are complex - ComplEx: entity and
        relation rows; RotatE: entity rows (its relation rows are d phases: coordinates); every other scorer:
        coordinates.  True on a scorer without [re | im] rows is refused; False: coordinates everywhere.
    """

    def __init__(self, p: float = 3.0, entity_coef: float = 0.0, relation_coef: Optional[float] = None,
                 complex_modulus: Optional[bool] = None) -> None:
        p = float(p)
        if not (math.isfinite(p) and p >= 1.0):
            raise ValueError(f"EmbeddingRegularizer: p = {p} is not a finite p >= 1")
        entity_coef = float(entity_coef)
        relation_coef = entity_coef if relation_coef is None else float(relation_coef)
        for name, c in (("entity_coef", entity_coef), ("relation_coef", relation_coef)):
            if not (math.isfinite(c) and c >= 0.0):
                raise ValueError(f"EmbeddingRegularizer: {name} = {c} must be finite and >= 0")
        if complex_modulus is not None and not isinstance(complex_modulus, bool):
            raise TypeError("EmbeddingRegularizer: complex_modulus must be None, True or False")
        self.p = p
        self.entity_coef = entity_coef
        self.relation_coef = relation_coef
        self.complex_modulus = complex_modulus

    @classmethod
    def n3(cls, coef: float, relation_coef: Optional[float] = None) -> "EmbeddingRegularizer":
        """N3: cubed moduli (cubed absolute values on real scorers, e.g. DistMult-N3)."""
        return cls(3.0, coef, relation_coef)

    @classmethod
    def lp(cls, p: float, coef: float, relation_coef: Optional[float] = None) -> "EmbeddingRegularizer":
        """Lp on coordinates: sum_k |x_k|^p (`lp(2, c)`: squared L2 norm of the triples' rows)."""
        return cls(p, coef, relation_coef, complex_modulus=False)

    def modulus_flags(self, score_fn: Any) -> int:
        """`flags` of `bess_regularize_triples` for the rows of `score_fn` (refuses `complex_modulus=True` on a scorer
        whose rows are not [re | im])."""
        from besskge.scoring import ComplEx, RotatE

        if isinstance(score_fn, ComplEx):
            found = nat.REG_ENTITY_MODULUS | nat.REG_RELATION_MODULUS
        elif isinstance(score_fn, RotatE):
            found = nat.REG_ENTITY_MODULUS
        else:
            found = 0
        if self.complex_modulus is None:
            return found
        if self.complex_modulus and not found:
            raise ValueError(f"EmbeddingRegularizer(complex_modulus=True): the rows of {type(score_fn).__name__} are not "
                             "[re | im] (ComplEx, RotatE)")
        return found if self.complex_modulus else 0

    def resolved_modulus(self, score_fn: Any) -> Tuple[bool, bool]:
        """(moduli on entity rows?, moduli on relation rows?) for `score_fn`."""
        f = self.modulus_flags(score_fn)
        return bool(f & nat.REG_ENTITY_MODULUS), bool(f & nat.REG_RELATION_MODULUS)

    def __repr__(self) -> str:
        return (f"EmbeddingRegularizer(p={self.p}, entity_coef={self.entity_coef}, relation_coef={self.relation_coef}, "
                f"complex_modulus={self.complex_modulus})")
