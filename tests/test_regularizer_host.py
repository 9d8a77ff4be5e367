"""`besskge.regularizer.EmbeddingRegularizer` and the plumbing of `bess_regularize_triples` (no GPU needed): how
`complex_modulus` resolves per scorer, what is refused, the shorthands, the symbol / signature / plan registration of
the entry point, and that `BessKGE` still builds without the new keyword."""

import ctypes
import math

import pytest


def scorer(name, d=4):
    from besskge import scoring
    from besskge.sharding import Sharding

    sharding = Sharding.create(40, 1, seed=0)
    if name in ("TransE", "RotatE", "PairRE", "TripleRE"):
        return getattr(scoring, name)(True, 1, sharding, 5, d)
    return getattr(scoring, name)(True, sharding, 5, d)


def sampler(fn):
    from besskge.negative_sampler import RandomShardedNegativeSampler

    return RandomShardedNegativeSampler(4, fn.sharding, 0, "t", local_sampling=False, flat_negative_format=True)


@pytest.mark.parametrize("name,want", [("ComplEx", (True, True)), ("RotatE", (True, False)), ("TransE", (False, False)),
                                       ("DistMult", (False, False)), ("PairRE", (False, False))])
def test_complex_modulus_resolves_per_scorer(name, want):
    from besskge import _native as nat
    from besskge.regularizer import EmbeddingRegularizer

    fn = scorer(name)
    assert EmbeddingRegularizer(3.0, 0.1).resolved_modulus(fn) == want
    assert EmbeddingRegularizer(3.0, 0.1, complex_modulus=False).resolved_modulus(fn) == (False, False)
    if any(want):
        assert EmbeddingRegularizer(3.0, 0.1, complex_modulus=True).resolved_modulus(fn) == want
        flags = EmbeddingRegularizer(3.0, 0.1).modulus_flags(fn)
        assert flags == (nat.REG_ENTITY_MODULUS * want[0]) | (nat.REG_RELATION_MODULUS * want[1])
    else:
        with pytest.raises(ValueError, match="re | im"):
            EmbeddingRegularizer(3.0, 0.1, complex_modulus=True).modulus_flags(fn)


def test_constructor_defaults_and_shorthands():
    from besskge.regularizer import EmbeddingRegularizer

    r = EmbeddingRegularizer(entity_coef=0.2)
    assert (r.p, r.entity_coef, r.relation_coef, r.complex_modulus) == (3.0, 0.2, 0.2, None)
    r = EmbeddingRegularizer(2.5, 0.2, relation_coef=0.0)
    assert (r.p, r.entity_coef, r.relation_coef) == (2.5, 0.2, 0.0)
    r = EmbeddingRegularizer.n3(1e-3)
    assert (r.p, r.entity_coef, r.relation_coef, r.complex_modulus) == (3.0, 1e-3, 1e-3, None)
    r = EmbeddingRegularizer.lp(2, 0.5)
    assert (r.p, r.entity_coef, r.relation_coef, r.complex_modulus) == (2.0, 0.5, 0.5, False)
    assert EmbeddingRegularizer.lp(1, 0.5, relation_coef=0.25).relation_coef == 0.25
    assert "EmbeddingRegularizer" in repr(r)
    import besskge

    assert besskge.regularizer.EmbeddingRegularizer is EmbeddingRegularizer


@pytest.mark.parametrize("kw", [dict(p=0.5), dict(p=math.nan), dict(p=math.inf), dict(entity_coef=-1e-3),
                                dict(relation_coef=-1.0), dict(entity_coef=math.nan), dict(relation_coef=math.inf)])
def test_constructor_refusals(kw):
    from besskge.regularizer import EmbeddingRegularizer

    with pytest.raises(ValueError):
        EmbeddingRegularizer(**dict(dict(p=3.0, entity_coef=0.1), **kw))


def test_complex_modulus_must_be_a_flag():
    from besskge.regularizer import EmbeddingRegularizer

    with pytest.raises(TypeError):
        EmbeddingRegularizer(3.0, 0.1, complex_modulus=1)


def test_entry_point_is_exported_signed_and_known_to_plans():
    from besskge import _native as nat

    lib = nat.load()
    assert hasattr(lib, "bess_regularize_triples")
    sig = nat.SIGNATURES["bess_regularize_triples"]
    assert len(sig) == 24 and list(lib.bess_regularize_triples.argtypes) == sig
    assert sig[-1] is ctypes.c_void_p  # the stream
    assert [i for i, t in enumerate(sig) if t is ctypes.c_float] == [10, 11, 12, 13, 21]
    assert lib.bess_plan_knows(b"bess_regularize_triples") == 1
    assert lib.bess_version() == 3  # nothing existing moved


def host_call(**kw):
    """`bess_regularize_triples` with pointers that are never followed: every refusal comes before the launch."""
    from besskge import _native as nat

    lib = nat.load()
    d = nat.ModelDesc()
    d.dtype, d.width, d.rel_width = kw.pop("dtype", nat.F32), kw.pop("width", 8), kw.pop("rel_width", 8)
    a = dict(head=64, tail=64, rel=64, rel_idx=64, n=4, weight=64, weight_len=1, p=3.0, ec=0.1, rc=0.1, scale=1.0,
             flags=0, dh=64, dt=64, drel=64, terms=64, penalty=64, loss=0, factor=1.0, ticket=64)
    a.update(kw)
    rc = lib.bess_regularize_triples(ctypes.byref(d), a["head"], 0, a["tail"], 0, a["rel"], a["rel_idx"], a["n"],
                                     a["weight"], a["weight_len"], a["p"], a["ec"], a["rc"], a["scale"], a["flags"],
                                     a["dh"], a["dt"], a["drel"], a["terms"], a["penalty"], a["loss"], a["factor"],
                                     a["ticket"], None)
    buf = ctypes.create_string_buffer(512)
    lib.bess_last_error(buf, 512)
    return rc, buf.value.decode()


@pytest.mark.parametrize("kw,text", [
    (dict(p=0.99), "p >= 1"), (dict(p=math.nan), "p >= 1"), (dict(p=math.inf), "p >= 1"),
    (dict(ec=-0.1), "coefficients"), (dict(rc=-0.1), "coefficients"),
    (dict(flags=1, width=7, rel_width=7), "odd width"), (dict(flags=2, width=8, rel_width=5), "odd width"),
    (dict(weight_len=3), "weight_len"), (dict(weight_len=0), "weight_len"),
    (dict(dh=0), "d_head and d_tail"), (dict(dt=0), "d_head and d_tail"),
    (dict(drel=0), "d_rel_table"), (dict(flags=4), "flags"), (dict(dtype=7), "dtype"), (dict(n=0), "sizes"),
])
def test_entry_point_refusals_carry_a_code_and_a_text(kw, text):
    rc, msg = host_call(**kw)
    assert rc == -1, (rc, msg)  # BESS_EINVAL
    assert "regularize_triples" in msg and text in msg, msg


def test_model_constructor_with_and_without_the_keyword():
    from besskge.bess import EmbeddingMovingBessKGE, ScoreMovingBessKGE
    from besskge.loss import LogSigmoidLoss
    from besskge.regularizer import EmbeddingRegularizer

    fn = scorer("ComplEx")
    loss = LogSigmoidLoss(margin=1.0, negative_adversarial_sampling=False)
    # as before the keyword existed: by name, and positionally up to `augment_negative`
    m = EmbeddingMovingBessKGE(negative_sampler=sampler(fn), score_fn=fn, loss_fn=loss)
    assert m.regularizer is None
    m = EmbeddingMovingBessKGE(sampler(fn), fn, loss, None, False, False)
    assert m.regularizer is None
    reg = EmbeddingRegularizer.n3(1e-2)
    for cls in (EmbeddingMovingBessKGE, ScoreMovingBessKGE):
        m = cls(negative_sampler=sampler(fn), score_fn=fn, loss_fn=loss, regularizer=reg)
        assert m.regularizer is reg and m._regularizer_flags == 3
    # the last keyword, positionally
    assert EmbeddingMovingBessKGE(sampler(fn), fn, loss, None, False, False, reg).regularizer is reg


def test_model_refusals():
    from besskge.bess import EmbeddingMovingBessKGE
    from besskge.loss import LogSigmoidLoss
    from besskge.regularizer import EmbeddingRegularizer

    fn = scorer("TransE")
    with pytest.raises(ValueError, match="loss_fn"):
        EmbeddingMovingBessKGE(negative_sampler=sampler(fn), score_fn=fn, return_scores=True,
                               regularizer=EmbeddingRegularizer.n3(1e-2))
    with pytest.raises(ValueError, match="re | im"):
        EmbeddingMovingBessKGE(negative_sampler=sampler(fn), score_fn=fn,
                               loss_fn=LogSigmoidLoss(margin=1.0, negative_adversarial_sampling=False),
                               regularizer=EmbeddingRegularizer(3.0, 1e-2, complex_modulus=True))
