"""CPU: sos_wsod_amd.wgrad — the grad_scope bookkeeping, the queue every weight-gradient node of a counted parameter joins (with a
recording fake flush; no kernel runs), and the split planners pinned to the values they returned before they moved here."""
import pytest
import torch

import sos_wsod_amd.wgrad as wgrad


def test_grad_scope_bookkeeping_is_inert_outside_and_loud_about_unfinished_queues():
    """wgrad.grad_scope (host logic only): outside a scope the helpers do nothing; inside, a registered buffer is found again by key
    and shape (as an alias on the same storage, never the same tensor object), use counts add up, nested scopes restore the outer
    one, and leaving a scope with a queued-but-unfinished weight gradient raises instead of handing autograd a half-written
    buffer."""
    assert wgrad.active() is None
    buf = torch.zeros(4, 6)
    wgrad.note_grad(1, buf); wgrad.count_use(1)
    assert wgrad.pending_grad(1, (4, 6)) is None and wgrad.use_count(1) == 0
    with wgrad.grad_scope() as outer:
        wgrad.count_use("w"); wgrad.count_use("w"); wgrad.count_use("v")
        assert (wgrad.use_count("w"), wgrad.use_count("v"), wgrad.use_count("u")) == (2, 1, 0)
        assert wgrad.pending_grad("w", (4, 6)) is None
        wgrad.note_grad("w", buf)
        got = wgrad.pending_grad("w", (24,))
        assert got is not None and got is not buf and got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (24,)
        assert wgrad.pending_grad("w", (5, 5)) is None                      # another size: not this buffer
        with wgrad.grad_scope() as inner:
            assert wgrad.active() is inner and wgrad.pending_grad("w", (4, 6)) is None and wgrad.use_count("w") == 0
        assert wgrad.active() is outer and wgrad.use_count("w") == 2
    assert wgrad.active() is None

    def one_of_two_arrives():
        wgrad.count_use("w"); wgrad.count_use("w")
        assert wgrad.join("w", ("x", "dy"), ((2, 2),), (None,), "cpu", None) is not wgrad.NOT_QUEUED
    with pytest.raises(RuntimeError, match="never finished"):
        with wgrad.grad_scope():
            one_of_two_arrives()
    assert wgrad.active() is None
    with pytest.raises(ValueError):                                           # an exception inside the scope is not masked
        with wgrad.grad_scope():
            one_of_two_arrives()
            raise ValueError("boom")
    assert wgrad.active() is None


def test_counted_function_sees_the_callers_grad_mode_not_the_forwards():
    """wgrad.CountedFunction / wgrad.count_use: inside a Function.forward autograd has switched grad mode off whatever the caller's mode
    is, so `apply` records the caller's; a use is counted in a normal pass and NOT counted under torch.no_grad() (the teacher's pass
    builds no backward node: a counted use would leave a queued weight gradient unfinished).  Regression: testing
    torch.is_grad_enabled() inside the forward counted nothing at all and silently disabled every grouped weight-gradient launch of
    Stage 3."""
    class Twice(wgrad.CountedFunction):
        @staticmethod
        def forward(ctx, x):
            assert not torch.is_grad_enabled()                 # what the regression tested
            wgrad.count_use("w")
            return x * 2

        @staticmethod
        def backward(ctx, g):
            return g * 2
    x = torch.ones(3, requires_grad=True)
    with wgrad.grad_scope():
        y = Twice.apply(x)
        assert wgrad.use_count("w") == 1 and y.requires_grad
        with torch.no_grad():
            z = Twice.apply(x)
        assert wgrad.use_count("w") == 1 and not z.requires_grad
        Twice.apply(x)
        assert wgrad.use_count("w") == 2
        wgrad.count_use("direct")                              # the recorded mode is restored after every apply, the one under
        assert wgrad.use_count("direct") == 1                  # no_grad included: a count outside any forward sees "enabled"
    Twice.apply(x)                                               # outside a scope: inert
    assert wgrad.use_count("w") == 0


class _Flush:
    """records what join hands its flush and writes something recognisable into the buffers"""

    def __init__(self):
        self.calls = []

    def __call__(self, bufs, scales, uses):
        self.calls.append((bufs, scales, list(uses)))
        for b in bufs:
            b.fill_(float(len(uses)))


def _join(key, operands, flush, force=False, shapes=((2, 3), (4,)), scales=("s0", None)):
    return wgrad.join(key, operands, shapes, scales, torch.device("cpu"), flush, force=force)


def test_join_three_uses_flush_once_on_the_last_in_arrival_order():
    flush = _Flush()
    with wgrad.grad_scope():
        for _ in range(3):
            wgrad.count_use("w")
        first = _join("w", "a", flush)
        assert isinstance(first, list) and [tuple(t.shape) for t in first] == [(2, 3), (4,)]
        assert all(t.dtype == torch.float32 for t in first)
        assert _join("w", "b", flush) is None and not flush.calls
        assert _join("w", "c", flush) is None
        assert len(flush.calls) == 1
        bufs, scales, uses = flush.calls[0]
        assert uses == ["a", "b", "c"] and tuple(scales) == ("s0", None)
        # what the first arrival was handed aliases the queue's storage (it sees the flush's result) but is another tensor object
        for got, kept in zip(first, bufs):
            assert got is not kept and got.data_ptr() == kept.data_ptr() and bool((got == 3.0).all())
        wgrad.finish()                                          # nothing left over


def test_join_declines_a_single_use_unless_forced():
    flush = _Flush()
    with wgrad.grad_scope():
        wgrad.count_use("w"); wgrad.count_use("f")
        assert _join("w", "a", flush) is wgrad.NOT_QUEUED
        assert _join(None, "a", flush, force=True) is wgrad.NOT_QUEUED
        assert _join("never counted", "a", flush, force=True) is wgrad.NOT_QUEUED
        assert not flush.calls
        got = _join("f", "a", flush, force=True)                # one use, forced: queued and flushed at once
        assert isinstance(got, list) and len(flush.calls) == 1 and flush.calls[0][2] == ["a"] and bool((got[0] == 1.0).all())
    assert _join("w", "a", flush, force=True) is wgrad.NOT_QUEUED and len(flush.calls) == 1      # outside a scope


def test_join_arrivals_without_operands():
    flush = _Flush()
    with wgrad.grad_scope():
        wgrad.count_use("e"); wgrad.count_use("e")
        first = _join("e", None, flush)
        for t in first:
            t.fill_(float("nan"))
        assert _join("e", None, flush) is None
        assert not flush.calls and all(bool((t == 0).all()) for t in first)       # nobody brought operands: zero-filled, no flush
        for _ in range(3):
            wgrad.count_use("s")
        _join("s", None, flush); _join("s", "b", flush); _join("s", None, flush)
        assert len(flush.calls) == 1 and flush.calls[0][2] == ["b"]               # the flush sees only the uses that brought some


def test_finish_raises_once_leaves_the_scope_clean_and_is_inert_outside():
    flush = _Flush()
    wgrad.finish()                                                  # outside a scope: nothing
    with wgrad.grad_scope():
        wgrad.finish()                                              # nothing queued
        wgrad.count_use("w"); wgrad.count_use("w")
        _join("w", "a", flush)
        with pytest.raises(RuntimeError, match="never finished"):
            wgrad.finish()
        wgrad.finish()                                              # the scope was emptied: silent, and so is leaving it
        assert wgrad.use_count("w") == 0 and not flush.calls
    assert wgrad.active() is None


# ---------------------------------------------------------------------------------------------------------- planners
def _backbone(h8, w8, nb=4, n=2):
    """(n, H, W, cin, cout, dilation) of the Stage-1 backbone's trainable convolutions in backward order, conv5_3 .. conv3_1 (conv3 maps
    are twice as wide and high as conv4 / conv5 ones), `nb` view batches of `n` images each"""
    h4, w4 = 2 * h8, 2 * w8
    layers = [(512, 512, h8, w8, 2)] * 3 + [(512, 512, h8, w8, 1)] * 2 + [(256, 512, h8, w8, 1)] + [(256, 256, h4, w4, 1)] * 2 + [(128, 256, h4, w4, 1)]
    return [(n, H, W, cin, cout, dil) for cin, cout, H, W, dil in layers for _ in range(nb)]


def _gemm_shapes(probs):
    return [(n * H * W, cout, 9 * cin) for n, H, W, cin, cout, dil in probs]


_PROBLEMS = {
    "headline": _backbone(63, 63),                                                   # 504 x 504 views, 4 view batches
    "recipe": [p for hw in ((99, 165), (104, 138)) for p in _backbone(*hw, nb=1)],   # a recipe pair of view sizes
    "tiny": [(1, 8, 8, 64, 64, 1), (1, 9, 40, 64, 64, 1), (1, 12, 20, 128, 64, 2), (3, 2, 33, 64, 64, 1)],
}
# what the planners returned at the commit before they moved into wgrad.py (computed there, on the CPU)
_PLANS = [
    ("headline", "direct", [1] * 24 + [4] * 12),
    ("headline", 64, 96, [1] * 24 + [5] * 12),
    ("headline", 32, 112, [2] * 24 + [9] * 12),
    ("recipe", "direct", [2] * 6 + [9] * 3 + [2] * 6 + [7] * 3),
    ("recipe", 64, 160, [3] * 6 + [13] * 3 + [3] * 6 + [11] * 3),
    ("recipe", 32, 160, [6] * 6 + [26] * 3 + [6] * 6 + [22] * 3),
    ("tiny", "direct", [1, 1, 1, 1]),
    ("tiny", 64, 40, [1, 1, 1, 1]),
]
_RPN = [(n * H * W, 256, 9 * 256) for n in (2, 1) for H, W in ((200, 304), (100, 152), (50, 76), (25, 38), (13, 19))]   # 800 x 1216
_RES5 = [s for P in (1900, 950) for s in ((P, 512, 1024), (P, 2048, 512), (P, 2048, 1024))]     # conv1, conv3, shortcut; two passes
_GROUPED = [      # (shapes, K-tile, candidates or None = the default, target, splits)
    (_RPN, 64, wgrad.GROUP_TARGETS, 72, [26, 7, 2, 1, 1, 13, 3, 1, 1, 1]),
    (_RPN, 32, wgrad.GROUP_TARGETS, 72, [53, 13, 3, 1, 1, 26, 7, 2, 1, 1]),
    (_RES5, 64, None, 40, [1, 1, 1, 1, 1, 1]),
    (_RES5, 64, wgrad.GROUP_TARGETS_1X1, 16, [2, 2, 2, 1, 1, 1]),
    (_RES5, 32, None, 40, [2, 2, 2, 1, 1, 1]),
    (_RES5, 32, wgrad.GROUP_TARGETS_1X1, 32, [2, 2, 2, 1, 1, 1]),
]


def test_split_planners_return_what_they_returned_before_the_move():
    assert wgrad.GROUP_TARGETS == (8, 12, 16, 24, 32, 40, 48, 56, 64, 72, 80, 96, 112, 128, 160)
    assert wgrad.GROUP_TARGETS_1X1 == (4, 6) + wgrad.GROUP_TARGETS
    for name, kind, *want in _PLANS:
        probs = _PROBLEMS[name]
        if kind == "direct":
            assert wgrad.wgrad_direct_splits(probs) == want[0], name
        else:
            shapes = _gemm_shapes(probs)
            target = wgrad.wgrad_grouped_target(shapes, kind)
            assert target == want[0], (name, kind)
            assert [wgrad.wgrad_grouped_splits(s[0], kind, target) for s in shapes] == want[1], (name, kind)
    for shapes, bk, cand, target, splits in _GROUPED:
        got = wgrad.wgrad_grouped_target(shapes, bk) if cand is None else wgrad.wgrad_grouped_target(shapes, bk, candidates=cand)
        assert got == target, (shapes[0], bk)
        assert [wgrad.wgrad_grouped_splits(s[0], bk, got) for s in shapes] == splits
    nslab = [(7938, 1, 1), (7938, 4, 4), (31752, 8, 8), (32670, 2, 2), (64, 3, 1), (65, 2, 2), (1000, 7, 6), (1000, 16, 16)]
    assert [wgrad.wgrad_nslab(a, b) for a, b, _ in nslab] == [c for _, _, c in nslab] and wgrad.wgrad_nslab(1000, 7, 32) == 7
    assert wgrad.wgrad_direct_covers(_PROBLEMS["headline"], torch.bfloat16) and not wgrad.wgrad_direct_covers(_PROBLEMS["headline"], torch.float32)
    assert not wgrad.wgrad_direct_covers(_PROBLEMS["tiny"][-1:], torch.bfloat16)         # H = 2 < 8


def test_direct_splits_never_leave_a_split_shorter_than_eight_steps():
    """wgrad_direct_splits shrinks a split count while the slabs the kernel really writes (wgrad_nslab) would leave fewer than 8
    steps per item.  The first guess is already capped at steps // 8 and wgrad_nslab never exceeds the split count it is given, so
    no shape makes that loop run; what it guarantees is checked here over small and odd maps, for every target length it tries."""
    for cand in wgrad.wgrad_direct_splits.__defaults__[1]:
        for n, H, W in ((1, 8, 8), (1, 9, 40), (2, 8, 33), (3, 17, 65), (1, 64, 31), (6, 11, 97), (2, 99, 165)):
            ns = wgrad.wgrad_direct_splits([(n, H, W, 64, 64, 1)], candidates=(cand,))[0]
            steps, eff = n * ((W + 31) // 32) * H, wgrad.wgrad_nslab(n * H * W, ns)
            assert 1 <= eff <= ns and (eff == 1 or -(-steps // eff) >= 8), (cand, n, H, W, ns, eff)


def test_planner_cache_survives_its_own_eviction():
    probs = _PROBLEMS["recipe"]
    before = (wgrad.wgrad_direct_splits(probs), wgrad.wgrad_grouped_target(_gemm_shapes(probs), 64))
    for i in range(520):                                            # more distinct keys than the cache keeps
        wgrad.wgrad_grouped_target([(64 * (i + 1), 64, 64)], 64, n_cu=8, candidates=(8,))
    assert len(wgrad.PLAN_CACHE) <= 513
    assert (wgrad.wgrad_direct_splits(probs), wgrad.wgrad_grouped_target(_gemm_shapes(probs), 64)) == before == ([2] * 6 + [9] * 3 + [2] * 6 + [7] * 3, 160)
