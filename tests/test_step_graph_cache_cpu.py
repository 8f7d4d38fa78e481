"""CPU: trainer._GraphCache — the one signature -> capture table behind both step-graph users — driven with a fake capture callable;
and the set of SW_* environment variables the package reads, pinned."""
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _cache():
    from sos_wsod_amd.trainer import _GraphCache
    return _GraphCache()


class _Capture:
    """a capture callable that hands out numbered tokens and counts its calls"""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return ("token", self.calls)


def test_first_sight_none_second_captures_third_replays_same_token():
    c, cap = _cache(), _Capture()
    assert c.lookup("a", cap) is None and cap.calls == 0 and c.captures == 0
    tok = c.lookup("a", cap)
    assert tok == ("token", 1) and cap.calls == 1 and c.captures == 1
    assert c.lookup("a", cap) is tok and c.lookup("a", cap) is tok
    assert cap.calls == 1 and c.captures == 1 and c.evictions == 0 and c.replays == 0          # (the caller counts replays)


def test_least_recently_used_is_evicted_and_must_recur_twice():
    c, cap = _cache(), _Capture()
    n = c.MAX_GRAPHS
    for i in range(n):
        assert c.lookup(i, cap) is None
        assert c.lookup(i, cap) is not None
    assert c.lookup(0, cap) == ("token", 1)                                                   # 0 is now the most recently used: 1 is the oldest
    assert c.lookup("new", cap) is None and c.evictions == 0 and len(c.graphs) == n           # first sight evicts nothing
    assert c.lookup("new", cap) is not None
    assert c.evictions == 1 and len(c.graphs) == n and c.captures == n + 1
    assert 1 not in c.graphs and 0 in c.graphs and all(i in c.graphs for i in range(2, n))
    calls = cap.calls
    assert c.lookup(1, cap) is None and cap.calls == calls                                    # the evicted signature: two more sights
    assert c.lookup(1, cap) is not None and cap.calls == calls + 1
    assert c.evictions == 2 and 2 not in c.graphs


def test_declined_capture_evicts_nothing_and_stores_nothing():
    c, cap = _cache(), _Capture()
    for i in range(c.MAX_GRAPHS):
        c.lookup(i, cap); c.lookup(i, cap)
    live = list(c.graphs)
    declined = []

    def decline():
        declined.append(1)
        return None
    assert c.lookup("x", decline) is None and not declined
    assert c.lookup("x", decline) is None and c.lookup("x", decline) is None
    assert len(declined) == 2                                                                 # asked again at every later sight
    assert list(c.graphs) == live and "x" not in c.graphs and c.evictions == 0 and c.captures == c.MAX_GRAPHS
    assert c.lookup("x", cap) is not None and c.evictions == 1                                # once it can be captured, it is


def test_seen_is_emptied_past_its_bound():
    c, cap = _cache(), _Capture()
    assert c.MAX_SEEN == 4096
    for i in range(c.MAX_SEEN):
        assert c.lookup(i, cap) is None
    assert len(c.seen) == c.MAX_SEEN
    assert c.lookup("one more", cap) is None
    assert len(c.seen) == 0 and cap.calls == 0 and not c.graphs
    assert c.lookup(0, cap) is None                                                           # forgotten: first sight again


# the variables a test, the benchmark or INTEGRATION.md's option list uses; a new one has to be added here deliberately
SURVIVORS = {"SW_LIB_PATH", "SW_STEP_GRAPH", "SW_DDP_NATIVE", "SW_DDP_OVERLAP_UPDATE", "SW_DDP_FC1_PANELS", "SW_DDP_GRAD_COMPRESS",
             "SW_FUSE_FC1_UPDATE", "SW_FP32X3", "SW_FP32X3_CONV", "SW_S3_BACKBONE_GRAPH", "SW_BENCH_DEVICE", "SW_DIST_BACKEND"}
# of these, read by the callers of trainer.init_distributed(backend=...) — the benchmark and the DDP test workers — not by the package
READ_BY_CALLERS = {"SW_DIST_BACKEND"}

_ENV_ACCESS = [r"os\.environ\.(?:get|pop|setdefault)\(\s*[\"'](SW_\w+)[\"']", r"os\.environ\[\s*[\"'](SW_\w+)[\"']\s*\]",
               r"os\.getenv\(\s*[\"'](SW_\w+)[\"']", r"[\"'](SW_\w+)[\"']\s+(?:not\s+)?in\s+os\.environ"]


def _sw_reads(path):
    src = open(path).read()
    return {m for pat in _ENV_ACCESS for m in re.findall(pat, src)}


def test_package_reads_exactly_the_surviving_switches():
    pkg = os.path.join(ROOT, "sos-wsod_amd")
    found = set()
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                found |= _sw_reads(os.path.join(d, f))
    assert found == SURVIVORS - READ_BY_CALLERS, sorted(found ^ (SURVIVORS - READ_BY_CALLERS))
    assert READ_BY_CALLERS <= _sw_reads(os.path.join(ROOT, "bench.py"))
