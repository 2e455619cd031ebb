"""api.Scanner: four protocol-scan engines (one per demodulator front end) over the same rows, and the name of the
protocol each channel carries.  The rows, the front ends and the checker are those of tests/test_scan.py."""
import numpy as np
import pytest

from digiham_amd import _capi, api
from test_scan import FRONTS, N_SAMPLES, SOURCE, STAT, model, protocols, rows7      # noqa: F401  (fixtures)

WANT = ["dmr", "ysf", "nxdn", "dstar", "pocsag", None, None]


def test_constants():
    assert _capi.PROTO["scan"] == 6 and len(_capi.SCAN_PATTERNS) == 9 and _capi.EV_SCAN_HIT == 80
    assert api.SCAN_STAT_DTYPE == STAT and api.SCAN_STAT_DTYPE.itemsize == 16
    assert api.SCAN_FRONTS == FRONTS and list(api.SCAN_SOURCE) == SOURCE
    assert [name for name, _ in api.SCAN_FAMILIES] == WANT[:5]


@pytest.fixture(scope="module")
def merged(protocols):
    """what Scanner.stats() has to return after the seven rows, pushed whole: each pattern from its own front end"""
    _, _, want = protocols
    out = np.zeros((7, 9), STAT)
    for b in range(7):
        for pid in range(9):
            out[b, pid] = want[SOURCE[pid]][b][1][pid]
    return out


def test_scanner_names_the_protocols(ctx, protocols, merged):
    x, syms, want = protocols
    sc = api.Scanner(7, N_SAMPLES, ctx=ctx)
    assert sc.classify() == [None] * 7 and (sc.stats()["best_dist"] == 255).all()      # nothing pushed yet
    half = N_SAMPLES // 2
    sc.push(np.ascontiguousarray(x[:, :half]))
    first = sc.stats()
    # a ragged push that brings channel 2 nothing leaves its statistics where they were
    counts = np.full(7, N_SAMPLES - half, np.uint32); counts[2] = 0
    sc.push(np.ascontiguousarray(x[:, half:]), counts=counts)
    st = sc.stats()
    assert st[2].tobytes() == first[2].tobytes() and st[0]["hits"].sum() > first[0]["hits"].sum()
    counts[:] = 0; counts[2] = N_SAMPLES - half
    sc.push(np.ascontiguousarray(x[:, half:]), counts=counts)
    st = sc.stats()
    assert st.tobytes() == merged.tobytes()
    for f in FRONTS:                                      # every front end counts all nine patterns; stats() picks
        fs = sc.front_stats(f)
        for b in range(7):
            assert fs[b].tobytes() == want[f][b][1].tobytes(), (f, b)
    assert sc.classify() == WANT
    top = max(int(merged[b]["periodic"].sum()) for b in range(7))
    assert sc.classify(confirm=top + 1) == [None] * 7
    # the hits of the last push of a channel, each pattern from its own front end
    ev = sc.hits(2)
    w = want["narrow20"][2][0]
    w = w[w["a"] == 5]
    n_half = model(_symbols_until(ctx, x[2], "narrow20", half))[0]
    assert len(ev[ev["a"] == 5]) and ev[ev["a"] == 5].tobytes() == w[len(n_half[n_half["a"] == 5]):].tobytes()
    sc.reset_channel(0)
    st = sc.stats()
    assert st[0]["hits"].sum() == 0 and (st[0]["best_dist"] == 255).all() and st[1:].tobytes() == merged[1:].tobytes()
    assert sc.classify() == [None] + WANT[1:]
    sc.reset()
    assert sc.classify() == [None] * 7
    sc.close()


def _symbols_until(ctx, row, front, n):
    eng = api.Engine(1, n, proto="none", ctx=ctx, **FRONTS[front])
    eng.push(np.ascontiguousarray(row[None, :n]))
    s, c = eng.symbols()
    eng.close()
    return s[0, :c[0]]


def test_scanner_takes_a_subset_of_front_ends(ctx, protocols):
    x, _, want = protocols
    sc = api.Scanner(7, N_SAMPLES, fronts=("narrow20",), ctx=ctx)
    sc.push(x)
    st = sc.stats()
    for b in range(7):
        assert st[b, 5].tobytes() == want["narrow20"][b][1][5].tobytes()
    assert st["hits"][:, [0, 1, 2, 3, 4, 6, 7, 8]].sum() == 0
    assert sc.classify() == [None, None, "nxdn", None, None, None, None]
    sc.close()
