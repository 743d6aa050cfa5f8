"""tests/spec_top.py (DESIGN.md section 2 rule 11) against two restatements that share no code with it: a plain-Python sorted()
over tuples, and a Python model of the kernels' selection — three histogram passes over 11 / 11 / 10 bits from the top, the digit
that holds the wanted rank, the threshold T and the number t of ties to take — so that the algorithm is checked before any kernel
runs.  No GPU needed."""
import random

import numpy as np
import pytest

import spec_top as spec

NONE = 0xFFFFFFFF


def plain(A, load, H, n, flags, node, min_key, cap):
    """the rule, row by row"""
    cand = []
    for r in range(n):
        k = (0 if H is None else int(H[r])) if flags & 1 else int(load[r])
        if k < min_key:
            continue
        if flags & 2 and int(A[r]) == NONE:
            continue
        if flags & 4 and int(A[r]) != node:
            continue
        cand.append((k, r))
    listed = sorted(cand, key=lambda kr: (-kr[0], kr[1]))[:cap]
    return ([r for _, r in listed], [k for k, _ in listed], [int(A[r]) for _, r in listed], len(cand), sum(k for k, _ in cand))


def radix_select(keys, cap):
    """keys: the candidates' keys (more than cap of them) -> (T, t): `cap` keys are >= T, exactly t of the listed ones equal T.
    Digit by digit from the top: a histogram of the keys that agree with the digits chosen so far, then the bin, counted from
    the top bin down, in which the running count first reaches the rank that is still wanted."""
    assert len(keys) > cap >= 1
    prefix, want, shift = 0, cap, 32
    for bits in (11, 11, 10):
        shift -= bits
        hist = [0] * (1 << bits)
        for k in keys:
            if (k >> (shift + bits)) == prefix:
                hist[(k >> shift) & ((1 << bits) - 1)] += 1
        run = 0
        for b in range((1 << bits) - 1, -1, -1):
            if run < want <= run + hist[b]:
                prefix, want = (prefix << bits) | b, want - run
                break
            run += hist[b]
        else:
            raise AssertionError("the bins never reach the wanted rank")
    return prefix, want


def columns(rng, n, m, kind):
    A = rng.integers(0, m, n, dtype=np.uint32)
    A[rng.random(n) < 0.3] = NONE
    if kind == "equal":
        K = np.full(n, 7, np.uint32)
    elif kind == "two":
        K = rng.choice(np.array([3, 0x80000001], np.uint32), n)
    elif kind == "low":
        K = (0x12345400 + rng.integers(0, 1024, n)).astype(np.uint32)
    elif kind == "mid":
        K = (0x40000155 + (rng.integers(0, 2048, n) << 10)).astype(np.uint32)
    elif kind == "top":
        K = ((rng.integers(0, 2048, n) << 21) + 0x1ABCDE).astype(np.uint32)
    elif kind == "ends":
        K = rng.choice(np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32), n)
    else:
        K = np.minimum(rng.zipf(1.3, n), 0xFFFFFFFF).astype(np.uint32)
    return A, K


KINDS = ["equal", "two", "low", "mid", "top", "ends", "zipf"]


@pytest.mark.parametrize("kind", KINDS)
def test_the_spec_is_the_plain_rule(kind):
    rng = np.random.default_rng(KINDS.index(kind))
    rnd = random.Random(kind)
    for n in (0, 1, 2, 257, 1500):
        A, K = columns(rng, n + 5, 5, kind)       # five hidden rows behind n
        H = None if rnd.random() < 0.3 else rng.integers(0, 4, n + 5, dtype=np.uint32)
        for flags in range(8):
            for cap in (0, 1, 64, 4096):
                node = rnd.randrange(5)
                min_key = rnd.choice([0, 1, int(K[0]) if n else 0, 0xFFFFFFFF])
                rows, keys, nodes, nc, ks = spec.top_rows(A, K, H, n, flags, node, min_key, cap)
                want = plain(A, K, H, n, flags, node, min_key, cap)
                assert (rows.tolist(), keys.tolist(), nodes.tolist(), nc, ks) == want, (kind, n, flags, cap, min_key)
                assert rows.dtype == keys.dtype == nodes.dtype == np.uint32


@pytest.mark.parametrize("kind", KINDS)
def test_the_digit_by_digit_selection_lists_what_the_spec_lists(kind):
    rng = np.random.default_rng(100 + KINDS.index(kind))
    for n in (2, 300, 5000):
        A, K = columns(rng, n, 3, kind)
        for flags, min_key in ((0, 0), (2, 0), (6, 1), (0, int(np.median(K)))):
            for cap in (1, 2, 63, 64, 65, 4095, 4096):
                rows, keys, nodes, nc, ks = spec.top_rows(A, K, None, n, flags, 1, min_key, cap)
                cand = [r for r in range(n) if K[r] >= min_key and (not flags & 2 or A[r] != NONE) and (not flags & 4 or A[r] == 1)]
                assert nc == len(cand)
                if nc <= cap:        # the early exit: everything is listed, no threshold is looked for
                    assert sorted(rows.tolist()) == cand
                    continue
                T, t = radix_select([int(K[r]) for r in cand], cap)
                above = [r for r in cand if K[r] > T]
                ties = [r for r in cand if K[r] == T]
                assert len(above) + t == cap and 1 <= t <= len(ties), (kind, n, cap, T, t)
                chosen = above + ties[:t]                     # the LOWEST rows among the ties
                chosen.sort(key=lambda r: ((int(K[r]) << 32) | (~r & 0xFFFFFFFF)), reverse=True)   # the final sort's composite key
                assert chosen == rows.tolist(), (kind, n, flags, cap)
                assert int(keys[-1]) == T


def test_the_string_layer_model_orders_by_load_then_row():
    rows = [("T", "a"), ("T", "b"), ("N\0", "x\0y"), ("T", "c"), ("T", "d")]
    where = {("T", "a"): "s0", ("T", "b"): "s1", ("N\0", "x\0y"): "s0", ("T", "d"): "s0"}
    load = {("T", "a"): 5, ("T", "b"): 9, ("N\0", "x\0y"): 5, ("T", "c"): 100, ("T", "d"): 1}
    assert spec.op_hottest(rows, where, load) == ([("T", "b", "s1", 9), ("T", "a", "s0", 5), ("N\0", "x\0y", "s0", 5), ("T", "d", "s0", 1)], 4)
    assert spec.op_hottest(rows, where, load, "s0", 2, 1) == ([("T", "a", "s0", 5)], 2)
    assert spec.op_hottest(rows, where, load, "nowhere") == ([], 0)
