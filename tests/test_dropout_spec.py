"""Statistics of the two dropout generators (tests/dropout_spec.py, the numpy statement of csrc/rng.h and csrc/attn_common.h), on the
CPU.  The reference's ``F.dropout(p)`` keeps every element i.i.d. with probability q = 1 - p; the parity tests of the dropout
sites evaluate the oracle with the mask the kernel exported, so only these tests can see a mask that keeps the right fraction
but is correlated, periodic or repeated.  tests/test_gpu_dropout_masks.py pins every site to the spec bit for bit.

Bounds.  For two independent Bernoulli(q) columns over n rows, the sample correlation r is approximately normal with mean 0
and sigma = 1 / sqrt(n) (the variance of a product of two independent standardised variables is 1, divided by n).  A kept
fraction over n elements has sigma = sqrt(q (1 - q) / n).  A single statistic is held to 5 sigma (false alarm ~6e-7); the
maximum over N statistics to 6 sigma: P(max |z| > 6) <= N * 2e-9, i.e. < 2e-5 for the 8,128 column pairs of a 128-column mask.
A real defect shows as a value that stays put as n grows (the attention's one-round element hash: 0.033 at 200 k and at 2 M
rows), while these bounds shrink as 1 / sqrt(n).  Every seed is fixed, so each test is deterministic.
"""
import functools

import numpy as np
import pytest

import dropout_spec as S

R = 200_000            # rows of the sampled masks
L = 128                # columns: every key of an attention row; 16 Philox groups of a row
SEED = 0x5DEECE66D1234567
PS = (0.1, 0.5)
GENS = ("philox", "attn")


def _mask(gen, p, seed=SEED, ctr=None, rows=R, **kw):
    if gen == "philox":
        return S.keep_mask(rows, L, seed, p, ctr)
    return S.attn_keep(1, 1, rows, L, seed, p, ctr, **kw).reshape(rows, L)


@functools.lru_cache(maxsize=None)
def _cached(gen, p, seed=SEED, ctr=None):
    m = _mask(gen, p, seed, ctr)
    m.setflags(write=False)
    return m


def _q(gen, p):
    """The exact keep probability of the spec's threshold."""
    return 1.0 - (S.tail_thr(p) / 65536.0 if gen == "philox" else S.attn_thr(p) / 4294967296.0)


def _corr(m):
    """[L, L] sample correlation matrix of the columns of a bool mask."""
    x = m.astype(np.float64)
    x -= x.mean(0)
    x /= x.std(0)
    return (x.T @ x) / x.shape[0]


def _pooled(a, b, q):
    """Correlation of the elements of two equally shaped masks, pooled over all elements (standardised with the exact q)."""
    s = np.sqrt(q * (1 - q))
    return float(np.mean(((a - q) / s) * ((b - q) / s)))


# ------------------------------------------------------------------------------------------------ thresholds
def test_thresholds_restate_the_library():
    """tail_thr / make_drop (16-bit) and attn_thr (32-bit): p as a C float, rounded, clamped; thr == 0 = no dropout."""
    assert S.tail_thr(0.1) == 6554 and S.tail_thr(0.5) == 32768 and S.tail_thr(0.0) == 0
    assert S.tail_thr(2.0 ** -18) == 0 and S.tail_thr(2.0 ** -16) == 1
    assert S.tail_thr(0.99999) == 65535
    assert S.attn_thr(0.1) == int(float(np.float32(0.1)) * 2 ** 32 + 0.5) and S.attn_thr(0.5) == 2 ** 31
    assert S.attn_thr(0.9999999999) == 2 ** 32 - 1 and S.attn_thr(0.0) == 0
    assert S.keep_mask(3, 64, SEED, 2.0 ** -18).all() and S.attn_keep(1, 2, 3, 5, SEED, 0.0).all()
    assert S.keep_scale(0.1) == np.float32(1.0) / np.float32(np.float32(1.0) - np.float32(0.1))


def test_eff_seed_is_the_64_bit_weyl_step():
    assert S.vlpet_eff_seed(5) == 5 and S.vlpet_eff_seed(5, 0) == 5
    assert S.vlpet_eff_seed(5, 1) == 5 + 0x9E3779B97F4A7C15
    big = (1 << 40) + 3
    assert S.vlpet_eff_seed(2 ** 64 - 1, big) == (2 ** 64 - 1 + big * 0x9E3779B97F4A7C15) % 2 ** 64


def test_philox_matches_the_published_structure():
    """keep8's bit j is lane j of the 128-bit output: word j >> 1, half j & 1; the mask is keep8 laid out group by group."""
    seed, thr = 0x0123456789ABCDEF, S.tail_thr(0.5)
    g = np.arange(40, dtype=np.uint64)
    o = S.philox7(g, np.zeros_like(g), seed & 0xFFFFFFFF, seed >> 32)
    bits = S.keep8(g, seed, thr)
    for j in range(8):
        u = (o[j >> 1] >> np.uint64(16 * (j & 1))) & np.uint64(0xFFFF)
        assert np.array_equal((bits >> j) & 1, (u >= thr).astype(np.uint32))
    m = S.keep_mask(5, 64, seed, 0.5)
    assert np.array_equal(m.reshape(-1, 8), ((bits[:, None] >> np.arange(8)) & 1).astype(bool))


def test_drop_pos_is_a_permutation_of_each_block_of_eight():
    G = np.arange(96)
    pos = S.drop_pos(G)
    assert sorted(pos.tolist()) == G.tolist()
    assert pos[:8].tolist() == [0, 4, 1, 5, 2, 6, 3, 7]
    m = _cached("philox", 0.1)[:7]
    pb = S.packed_bits(m)
    for G_ in range(L // 8):
        byte = pb[:, S.drop_pos(G_)]
        assert np.array_equal(((byte[:, None] >> np.arange(8)) & 1).astype(bool), m[:, 8 * G_:8 * G_ + 8])


# ------------------------------------------------------------------------------------------------ keep fractions
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("gen", GENS)
def test_keep_fraction_overall_equals_the_threshold(gen, p):
    m = _cached(gen, p)
    q = _q(gen, p)
    n = m.size
    assert abs(q - (1 - p)) <= 2.0 ** -16                              # the threshold is p rounded to the generator's resolution
    assert abs(m.mean() - q) <= 5 * np.sqrt(q * (1 - q) / n), (m.mean(), q)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("gen", GENS)
def test_keep_fraction_per_column_and_per_lane(gen, p):
    """Per column (n = R each, max over 128) and per lane of the 8-element group and per 16-bit half of a Philox word (a lane
    biased by how the 64-bit products are split would show here)."""
    m = _cached(gen, p)
    q = _q(gen, p)
    col = m.mean(0)
    assert np.abs(col - q).max() <= 6 * np.sqrt(q * (1 - q) / R), np.abs(col - q).max()
    lanes = m.reshape(R, L // 8, 8).mean(axis=(0, 1))
    assert np.abs(lanes - q).max() <= 6 * np.sqrt(q * (1 - q) / (R * L // 8)), lanes
    halves = m.reshape(R, L // 2, 2).mean(axis=(0, 1))
    assert np.abs(halves - q).max() <= 5 * np.sqrt(q * (1 - q) / (R * L // 2)), halves


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("gen", GENS)
def test_keep_count_per_row_is_binomial(gen, p):
    """Per row: the count over 128 elements is Binomial(128, q).  Its sample mean (5 sigma) and variance: the variance of a
    sample variance of n draws is about 2 v^2 / n, so the ratio to 128 q (1 - q) is held to 1 +- 5 sqrt(2 / R) -- rows that are
    all kept or all dropped together (a row-level correlation) inflate it."""
    m = _cached(gen, p)
    q = _q(gen, p)
    c = m.sum(1).astype(np.float64)
    v = L * q * (1 - q)
    assert abs(c.mean() - L * q) <= 5 * np.sqrt(v / R)
    assert abs(c.var() / v - 1) <= 5 * np.sqrt(2.0 / R), c.var() / v
    assert c.min() > 0


# ------------------------------------------------------------------------------------------------ correlations inside a mask
def _column_pair_worst(m):
    c = _corr(m)
    np.fill_diagonal(c, 0.0)
    i, j = np.unravel_index(np.abs(c).argmax(), c.shape)
    return abs(c[i, j]), (int(i), int(j)), c


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("gen", GENS)
def test_column_pairs_are_uncorrelated(gen, p):
    """All 8,128 column pairs of an [R, 128] mask: max |r| <= 6 / sqrt(R) = 0.0134.  Pooled lag-k correlation along a row (the mean
    of r over the 128 - k pairs (j, j + k)): sigma = 1 / sqrt(R (128 - k)), max over the 127 lags <= 6 sigma."""
    worst, at, c = _column_pair_worst(_cached(gen, p))
    assert worst <= 6 / np.sqrt(R), (worst, at)
    for k in range(1, L):
        lag = np.mean(np.diagonal(c, k))
        assert abs(lag) <= 6 / np.sqrt(R * (L - k)), (k, lag)


def test_column_pair_bound_catches_the_one_round_element_hash():
    """The attention's element hash before this check existed (one multiply-xorshift round after the Weyl step) fails the bound
    above by a wide margin: structured pairs, not noise (0.033 at 2 M rows as at 200 k)."""
    for p in PS:
        m = _mask("attn", p, elem=S.hash_elem_one_round, rkey=S.row_key_xor)
        worst, at, c = _column_pair_worst(m)
        assert worst > 2 * 6 / np.sqrt(R), (p, worst, at)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("gen", GENS)
def test_rows_are_uncorrelated(gen, p):
    """Adjacent rows, and rows whose indices differ in one bit (row_key once mixed the row index into the seed with a xor):
    pooled over all elements of the row pairs, sigma = 1 / sqrt(pairs * 128), each <= 6 sigma (18 statistics)."""
    m = _cached(gen, p)
    q = _q(gen, p)
    r = _pooled(m[:-1], m[1:], q)
    assert abs(r) <= 6 / np.sqrt((R - 1) * L), r
    rows = np.arange(R)
    for b in range(17):
        partner = rows ^ (1 << b)
        sel = (partner < R) & (rows < partner)
        r = _pooled(m[rows[sel]], m[partner[sel]], q)
        assert abs(r) <= 6 / np.sqrt(sel.sum() * L), (b, r)


# ------------------------------------------------------------------------------------------------ correlations across seeds
def _cross_checks(a, b, q, what):
    """Two masks of different seeds: element for element (pooled, 5 sigma), column for column (max of 128, 6 sigma), and row r of
    one against rows r ^ 1, r + 1 of the other (the same rows in another order would show as a correlation of 1)."""
    r = _pooled(a, b, q)
    assert abs(r) <= 5 / np.sqrt(a.size), (what, r)
    s = np.sqrt(q * (1 - q))
    col = np.mean(((a - q) / s) * ((b - q) / s), axis=0)
    assert np.abs(col).max() <= 6 / np.sqrt(a.shape[0]), (what, np.abs(col).max())
    rows = np.arange(a.shape[0])
    r1 = _pooled(a, b[rows ^ 1], q)
    assert abs(r1) <= 5 / np.sqrt(a.size), (what, "row ^ 1", r1)
    r2 = _pooled(a[:-1], b[1:], q)
    assert abs(r2) <= 5 / np.sqrt(a.size), (what, "row + 1", r2)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("gen", GENS)
def test_consecutive_replay_steps_are_independent(gen, p):
    """Graph replay: step t and t + 1 differ by the counter (seed + ctr * G, vlpet_eff_seed) -- ctr 0 / 1 and 2^40 + 3 / 2^40 + 4."""
    q = _q(gen, p)
    _cross_checks(_cached(gen, p, SEED, 0), _cached(gen, p, SEED, 1), q, "ctr 0 / 1")
    big = (1 << 40) + 3
    _cross_checks(_cached(gen, p, SEED, big), _cached(gen, p, SEED, big + 1), q, "ctr 2^40 + 3 / + 4")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("gen", GENS)
def test_low_bit_seed_neighbours_are_independent(gen, p):
    q = _q(gen, p)
    _cross_checks(_cached(gen, p, SEED), _cached(gen, p, SEED ^ 1), q, "seed ^ 1")
    _cross_checks(_cached(gen, p, SEED), _cached(gen, p, SEED ^ (1 << 32)), q, "seed ^ 2^32")


def test_seed_neighbour_check_catches_the_xor_row_key():
    """The attention's row key before this check existed hashed seed_lo ^ row: seeds s and s ^ 1 then gave the same rows, pairwise
    swapped (row r of one = row r ^ 1 of the other)."""
    a = _mask("attn", 0.1, SEED, rows=4096, rkey=S.row_key_xor)
    b = _mask("attn", 0.1, SEED ^ 1, rows=4096, rkey=S.row_key_xor)
    assert np.array_equal(a, b[np.arange(4096) ^ 1])
    with pytest.raises(AssertionError):
        _cross_checks(a, b, _q("attn", 0.1), "xor row key")
