"""CPU: the referee of the epoch sampler's tests -- draws_ref.choice_row(seed, e, 0, G, G) as perm_e and the rank windows
(t * world + rank) * D ... + D of it (INTEGRATION.md "Epoch-exact label sampling") -- checked for what the contract promises of it:
a permutation per epoch, windows that partition its prefix and drop the tail, and, for a fixed label, a turn that is uniform over
the T turns of an epoch."""
import numpy as np
import pytest

import draws_ref as R

SEED = 0x0123456789ABCDEF


def _window(perm, t, rank, world, D):
    r0 = (t * world + rank) * D
    return perm[r0:r0 + D]


@pytest.mark.parametrize("G", [1, 2, 5, 257, 4096, 4097, 70000])
def test_the_permutation_is_a_permutation_and_epochs_differ(G):
    p0, p1 = R.choice_row(SEED, 0, 0, G, G), R.choice_row(SEED, 1, 0, G, G)
    for p in (p0, p1):
        assert p.dtype == np.int32 and np.array_equal(np.sort(p), np.arange(G))
    assert G < 5 or not np.array_equal(p0, p1)
    assert np.array_equal(R.choice_row(SEED, 0, 0, G, min(G, 48)), p0[:min(G, 48)])          # a draw of N is the prefix of the order


@pytest.mark.parametrize("G,D,world", [(5, 2, 1), (100, 7, 1), (1000, 16, 3), (5000, 1024, 1), (5000, 48, 2), (4096, 2048, 2)])
def test_the_windows_of_an_epoch_partition_its_prefix(G, D, world):
    T = G // (D * world)
    perm = R.choice_row(SEED, 4, 0, G, G)
    wins = [_window(perm, t, r, world, D) for t in range(T) for r in range(world)]
    assert all(len(w) == D for w in wins)
    cat = np.concatenate(wins)
    assert np.array_equal(cat, perm[:T * D * world]) and len(np.unique(cat)) == T * D * world
    assert G - T * D * world < D * world                               # the dropped tail never fills a step
    assert len(_window(perm, T, 0, world, D)) < D or world > 1         # there is no turn T


def test_the_turn_of_a_fixed_label_is_uniform_over_the_epochs_turns():
    """G = 50, D = 4: T = 12 turns and a tail of 2.  Over 3000 epochs the turn of label j (the epochs that drop it set aside) is
    tested against the uniform distribution over T with Pearson's chi-square at the 99.9 % level (11 degrees of freedom: 31.264),
    and the drop count against its binomial mean within 3.3 sigma (the same level, two-sided)."""
    G, D, E = 50, 4, 3000
    T = G // D
    rank_of = np.empty((E, G), dtype=np.int64)
    for e in range(E):
        rank_of[e, R.choice_row(SEED, e, 0, G, G)] = np.arange(G)
    for j in (0, 17, 49):
        turn = rank_of[:, j] // D
        kept = turn[turn < T]
        dropped = E - len(kept)
        mean, sd = E * (G - T * D) / G, np.sqrt(E * (G - T * D) / G * (1 - (G - T * D) / G))
        assert abs(dropped - mean) <= 3.3 * sd, (j, dropped, mean)
        obs = np.bincount(kept, minlength=T)
        exp = len(kept) / T
        chi2 = float(((obs - exp) ** 2 / exp).sum())
        print("label %d: dropped %d of %d (mean %.1f), chi-square over %d turns %.2f" % (j, dropped, E, mean, T, chi2))
        assert chi2 <= 31.264, (j, chi2)
