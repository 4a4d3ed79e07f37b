"""The walk in bound order of the 64-channel kNN search (csrc/lpd_knn.hip, knn7_kernel<SORTED>), stated in numpy
(tests/knn_sorted_walk_ref.py) and checked without a GPU:

  * the image: over every 16-bit pattern the bound table can hold -- 0x7f80 ("visit"), +0, -0 and every finite negative bf16 -- the
    unsigned order of the image is exactly the descending order of the float values (+0 before -0, which are equal as floats);
  * the key: for random tables the argsort of (score image << 8 | tile) equals a plain Python sort by (-bound as float, tile), the
    bound of a tile being the largest entry of its 32 queries;
  * the stop rule: on random tables and random non-decreasing threshold sequences the walk never ends in front of a tile that the
    per-query test (ub >= threshold, any query) would have passed, then or at any later time;
  * the oracle alone: the rows whose top-k hangs on a tie rule stay under 1 % for every cloud the GPU test compares with it.
"""
import numpy as np
import pytest

import knn_sorted_walk_ref as ref
from oracle import lpd_oracle as orc

FINITE_NEG = np.arange(0x8001, 0xff80, dtype=np.uint32)                  # -tiny (denormal) .. the most negative finite bf16
PATTERNS = np.concatenate([[ref.INF_BITS, 0x0000, 0x8000], FINITE_NEG]).astype(np.uint32)


def test_image_orders_every_pattern_the_table_holds():
    val = ref.bits_to_f32(PATTERNS).astype(np.float64)
    assert np.isposinf(val[0]) and np.isfinite(val[1:]).all() and (val[1:] <= 0).all()
    img = ref.image(PATTERNS)
    assert img.max() <= 0xffff and np.unique(img).size == img.size, "the image is 16 bits wide and one to one"
    assert np.array_equal(ref.image(img), PATTERNS), "the image is its own inverse"
    by_img = np.argsort(img, kind="stable")
    v = val[by_img]
    assert (np.diff(v) <= 0).all(), "ascending image, descending float"
    # ... and exactly: a strictly larger float has a strictly smaller image (the only equal floats are +0 and -0: +0 first)
    a, b = np.meshgrid(np.arange(0, PATTERNS.size, 97), np.arange(PATTERNS.size), indexing="ij")
    assert ((val[a] > val[b]) <= (img[a] < img[b])).all() and ((val[a] < val[b]) <= (img[a] > img[b])).all()
    assert [int(i) for i in ref.image([ref.INF_BITS, 0x0000, 0x8000, 0x8001, 0xff7f])] == [0x007f, 0x7fff, 0x8000, 0x8001, 0xff7f]


def random_table(rng, nt, zero):
    """[nt, 32] uint16 of table patterns: mostly finite negatives from a few magnitudes (many equal scores), some 0x7f80, some zeros of
    ONE sign per table (+0 and -0 are equal floats that the key tells apart: that corner is test_zero_signs below)"""
    pool = np.concatenate([rng.choice(FINITE_NEG, 6), rng.integers(0xc000, 0xc400, 6), [ref.INF_BITS, zero]]).astype(np.uint16)
    t = rng.choice(pool, (nt, 32))
    t[rng.random(nt) < 0.3] = rng.choice(pool)          # whole rows equal: ties between tiles
    return t


@pytest.mark.parametrize("nt", [1, 2, 3, 13, 64, 65, 128])
def test_key_sorts_like_bound_then_tile(nt):
    rng = np.random.default_rng(100 + nt)
    for trial in range(20):
        t = random_table(rng, nt, 0x0000 if trial % 2 else 0x8000)
        bound = ref.bits_to_f32(t).max(-1)
        want = sorted(range(nt), key=lambda T: (-float(bound[T]), T))
        got = np.argsort(ref.keys(t), kind="stable")
        assert got.tolist() == want
        assert ((np.sort(ref.keys(t)) & 0xff) == got).all(), "the tile rides in the key's low byte"


def test_zero_signs():
    t = np.full((3, 32), 0xc000, np.uint16)
    t[0, 5] = 0x8000                                    # tile 0: best bound -0
    t[1, 7] = 0x0000                                    # tile 1: best bound +0
    t[2, 0] = ref.INF_BITS
    assert np.argsort(ref.keys(t)).tolist() == [2, 1, 0]


@pytest.mark.parametrize("nt", [2, 13, 65, 128])
def test_stop_never_hides_a_tile_some_query_would_visit(nt):
    rng = np.random.default_rng(200 + nt)
    stops = 0
    for trial in range(30):
        t = random_table(rng, nt, 0x8000)
        ub = ref.bits_to_f32(t)                                              # [T, q]
        real = np.arange(32) < (32 if trial % 3 else rng.integers(1, 32))    # the last tile of a cloud may hold padded queries
        # thresholds per walk step: -inf while a list is not full, then values around the table's, never falling; padded: +inf
        steps = nt + 1
        # (the best of m draws from the table: small m leaves loose thresholds, large m tight ones that end the walk early)
        raw = ref.bits_to_f32(rng.choice(t.reshape(-1), (int(rng.integers(1, 40)), steps, 32))).astype(np.float32)
        raw[np.isposinf(raw)] = 0.0
        raw = raw.max(0)
        raw[np.arange(steps)[:, None] < rng.integers(1, max(2, steps // 2) + 1, 32)[None, :]] = -np.inf
        thr = np.maximum.accumulate(raw, 0)
        thr[:, ~real] = np.inf
        order = np.sort(ref.keys(t))
        tiles = (order & 0xff).astype(int)
        for step in range(steps):                                            # the walk stands at position `step` when it tests
            pos = step if step < nt else nt - 1
            thr_min = thr[step, real].min()
            stop = ref.stop_position(order[pos:], thr_min) + pos
            if stop == pos and pos < nt:                                     # the walk ends here: nothing behind may pass, now or later
                stops += 1
                later = thr[step:]                                           # [s, q]
                hidden = ub[tiles[pos:]]                                     # [p, q]
                passes = hidden[None, :, :] >= later[:, None, :]
                assert not passes.any(), (trial, step, np.argwhere(passes)[:3].tolist())
            # a 0x7f80 score is never stepped over, whatever the threshold
            inf_pos = np.nonzero((order >> 8) == ref.image(ref.INF_BITS))[0]
            if inf_pos.size:
                assert ref.stop_position(order, thr_min) > inf_pos.max()
    assert stops > 0, "the fixture never reaches the stop"


@pytest.mark.parametrize("name", [n for n in sorted(ref.CASES)])
def test_oracle_tie_rows_under_one_percent(name):
    B, N, k = ref.CASES[name]
    x = ref.cloud(name)
    clouds = range(1, B) if name in ("identical", "nonfinite") else range(B)      # cloud 0 of these two is compared with the Z-curve walk only
    tie = orc.knn_tie_rows(x[list(clouds)], k)
    assert tie.mean() < 0.01, tie.mean()
