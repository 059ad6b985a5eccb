"""CPU: the one rule of the per-series caches of the likelihoods (ops._SeriesCache) on CPU tensors with an injected
``capturing`` answer, and the one rule for "a number or one value per draw" (ops._per_draw)."""
import gc
import weakref

import pytest
import torch

from exoplanet_amd import ops


class Capturing:
    def __init__(self):
        self.now = False

    def __call__(self):
        return self.now


@pytest.fixture
def cache():
    return ops._SeriesCache(capturing=Capturing())


def series(seed, n=12):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, dtype=torch.float64, generator=g), torch.rand(n, dtype=torch.float64, generator=g)


def lookup(cache, y, yerr, mean=0.0):
    made = []

    def make():
        made.append(True)
        return y - mean, y * y

    return cache.get((y, yerr, mean), make), bool(made)


def test_a_hit_returns_the_same_entry(cache):
    y, yerr = series(0)
    first, made = lookup(cache, y, yerr)
    assert made and first.sources[0] is y and first.sources[1] is yerr and torch.equal(first.value[1], y * y)
    again, made = lookup(cache, y, yerr)
    assert again is first and not made
    assert lookup(cache, y.detach(), yerr)[0] is first       # another object on the same storage, version and layout
    other, made = lookup(cache, y, yerr, mean=0.5)           # the numbers are part of the key
    assert made and other is not first
    assert lookup(cache, y, 0.1)[0] is lookup(cache, y, 0.1)[0]
    assert lookup(cache, y, None)[0] is not lookup(cache, y, 0.0)[0]


def test_a_source_edited_in_place_misses(cache):
    y, yerr = series(1)
    first, _ = lookup(cache, y, yerr)
    y.add_(1.0)
    second, made = lookup(cache, y, yerr)
    assert made and second is not first and torch.equal(second.value[0], y)
    yerr.mul_(2.0)
    assert lookup(cache, y, yerr)[1]


def test_a_view_of_the_same_address_and_size_with_another_stride_misses(cache):
    base = torch.arange(24, dtype=torch.float64)
    a, b = base[:12], base[:24:2]
    assert a.data_ptr() == b.data_ptr() and a.numel() == b.numel() and a._version == b._version
    first, _ = lookup(cache, a, 1.0)
    second, made = lookup(cache, b, 1.0)
    assert made and second is not first
    third, made = lookup(cache, base[:12].reshape(3, 4), 1.0)    # ... and with another shape
    assert made and third is not first


def test_a_fifth_series_empties_the_store_and_a_held_entry_keeps_its_sources(cache):
    y, yerr = series(2)
    ref = weakref.ref(y)
    held, _ = lookup(cache, y, yerr)
    del y
    for seed in range(3):
        lookup(cache, *series(10 + seed))
    assert len(cache.kept) == 4
    lookup(cache, *series(20))
    assert len(cache.kept) == 1 and not cache.pinned
    gc.collect()
    assert ref() is not None and ref() is held.sources[0]       # the entry, not the store, keeps the address taken
    again, made = lookup(cache, ref(), yerr)
    assert made and again is not held
    del held, again
    for seed in range(4):
        lookup(cache, *series(30 + seed))
    gc.collect()
    assert ref() is None


def test_a_miss_while_capturing_is_returned_but_not_stored(cache):
    y, yerr = series(3)
    cache.capturing.now = True
    entry, made = lookup(cache, y, yerr)
    assert made and torch.equal(entry.value[0], y)
    assert not cache.kept and not cache.pinned
    assert lookup(cache, y, yerr)[1]
    cache.capturing.now = False
    assert lookup(cache, y, yerr)[1] and len(cache.kept) == 1


def test_a_hit_while_capturing_pins_the_entry(cache):
    y, yerr = series(4)
    warm, _ = lookup(cache, y, yerr)
    ptrs = [x.data_ptr() for x in warm.value]
    cache.capturing.now = True
    captured, made = lookup(cache, y, yerr)
    cache.capturing.now = False
    assert captured is warm and not made
    assert list(cache.pinned.values()) == [warm] and not cache.kept      # moved: it no longer counts against the four
    others = [series(40 + seed) for seed in range(6)]
    for other in others:
        lookup(cache, *other)
    assert len(cache.kept) == 2 and list(cache.pinned.values()) == [warm]
    for now in (False, True):
        cache.capturing.now = now
        again, made = lookup(cache, y, yerr)
        assert again is warm and not made and [x.data_ptr() for x in again.value] == ptrs


def test_a_constant_handed_to_a_capture_stays(monkeypatch):
    consts = ops._SeriesCache(capacity=256, capturing=Capturing())
    monkeypatch.setattr(ops, "_CONSTS", consts)
    one = ops._const(1.0, "cpu")
    assert one is ops._const(1, torch.device("cpu")) and one.tolist() == [1.0]
    consts.capturing.now = True
    assert ops._const(1.0, "cpu") is one
    consts.capturing.now = False
    for k in range(300):
        ops._const(2.0 + k, "cpu")
    assert len(consts.kept) <= 256 and ops._const(1.0, "cpu") is one


# D = 3: what the three helpers that _per_draw replaces took and refused (the white-noise likelihood's, the astrometric
# likelihood's, and -- columns -- the radial-velocity likelihood's).  None: refused.
NUMBER, SCALAR = "number", ()
PER_DRAW = [  # argument, shape of the result, shape of the result with columns=True
    (NUMBER, (1,), (1, 1)),
    (SCALAR, (1,), (1, 1)),
    ((1,), (1,), (1, 1)),
    ((3,), (3,), (3, 1)),
    ((3, 1), (3,), (3, 1)),
    ((1, 1), (1,), (1, 1)),
    ((2,), None, None),
    ((3, 2), None, (3, 2)),
]


@pytest.mark.parametrize("columns", [False, True])
@pytest.mark.parametrize("arg,flat,wide", PER_DRAW, ids=[str(row[0]) for row in PER_DRAW])
def test_per_draw_shapes(monkeypatch, arg, flat, wide, columns):
    monkeypatch.setattr(ops, "_CONSTS", ops._SeriesCache(capacity=256, capturing=lambda: False))
    x = 0.25 if arg == NUMBER else torch.arange(1.0, 1.0 + torch.Size(arg).numel(), dtype=torch.float64).reshape(arg)
    want = wide if columns else flat
    what = "some likelihood"
    if want is None:
        count = r"some likelihood: `x` holds 2 draws, the parameters 3 -- one value, or one per draw"
        shape = r"some likelihood: `x` has shape \(3, 2\) -- a number, one value per draw, or \(draws,\) or \(draws, 1\)"
        with pytest.raises(ValueError, match=count if arg == (2,) else shape):
            ops._per_draw(x, "x", 3, "cpu", what, columns=columns)
        return
    got = ops._per_draw(x, "x", 3, "cpu", what, columns=columns)
    assert tuple(got.shape) == want and got.dtype == torch.float64
    assert torch.equal(got.reshape(-1), torch.tensor([0.25], dtype=torch.float64) if arg == NUMBER else x.reshape(-1))


def test_data_that_requires_grad_is_refused_by_name():
    y, yerr = series(5)
    ops._refuse_data_grad("some likelihood", "the orbit", "torch", y=y, yerr=yerr, mean=0.0, none=None)
    yerr.requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"some likelihood: `yerr` requires grad, and the fused kernels differentiate "
                                                  r"the orbit only; use torch"):
        ops._refuse_data_grad("some likelihood", "the orbit", "torch", y=y, yerr=yerr)
    with torch.no_grad():
        ops._refuse_data_grad("some likelihood", "the orbit", "torch", y=y, yerr=yerr)
        assert not ops.needs_grad(yerr)
    assert ops.needs_grad(yerr) and not ops.needs_grad(y) and not ops.needs_grad(1.0)
