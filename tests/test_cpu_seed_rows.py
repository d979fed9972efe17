"""core.pcg64_row / core.seed_rows: the one place where a numpy PCG64 becomes the words of a device stream row ([state_hi, state_lo, inc_hi, inc_lo] and, for the mazes,
numpy's buffered 32-bit half).  No GPU, no native library."""
import numpy as np
import pytest

from gymnasium_robotics_amd.core import np_random, pcg64_row, seed_rows

SEEDS = [0, 1, 12345, 2**63 - 1]
MASK = (1 << 64) - 1


def _words(s):
    st = np.random.PCG64(np.random.SeedSequence(s)).state["state"]
    return [st["state"] >> 64, st["state"] & MASK, st["inc"] >> 64, st["inc"] & MASK]


@pytest.mark.parametrize("buffered", [False, True])
def test_seed_rows_are_the_words_of_numpys_seeded_pcg64(buffered):
    rows = seed_rows(SEEDS, buffered=buffered)
    assert rows.dtype == np.uint64 and rows.shape == (len(SEEDS), 5 if buffered else 4)
    for row, s in zip(rows, SEEDS):
        assert [int(x) for x in row[:4]] == _words(s)
        if buffered:
            assert int(row[4]) == 0      # a freshly seeded generator holds no buffered 32-bit draw


@pytest.mark.parametrize("buffered", [False, True])
def test_a_generator_rebuilt_from_a_row_continues_the_seeded_stream(buffered):
    for row, s in zip(seed_rows(SEEDS, buffered=buffered), SEEDS):
        a = [int(x) for x in row]
        bg = np.random.PCG64()      # as GoalVecEnv.world_rng rebuilds it
        st = bg.state
        st["state"] = {"state": (a[0] << 64) | a[1], "inc": (a[2] << 64) | a[3]}
        if len(a) > 4:
            st["has_uint32"], st["uinteger"] = int(a[4] >> 32), int(a[4] & 0xFFFFFFFF)
        bg.state = st
        g, ref = np.random.Generator(bg), np_random(s)[0]
        assert np.array_equal(g.uniform(size=4), ref.uniform(size=4))
        assert int(g.integers(0, 2**32)) == int(ref.integers(0, 2**32))


def test_pcg64_row_carries_the_buffered_half_of_a_32_bit_draw():
    g = np_random(7)[0]
    g.integers(0, 2**32 - 1, dtype=np.uint32)      # one 32-bit draw: numpy keeps the other half of the 64-bit output
    st = g.bit_generator.state
    assert st["has_uint32"] == 1
    row = pcg64_row(st, buffered=True)
    assert len(row) == 5 and all(isinstance(x, int) for x in row)
    assert row[4] >> 32 == 1 and row[4] & 0xFFFFFFFF == int(st["uinteger"])
    assert row[:4] == pcg64_row(st) == [st["state"]["state"] >> 64, st["state"]["state"] & MASK, st["state"]["inc"] >> 64, st["state"]["inc"] & MASK]


@pytest.mark.parametrize("bad", [-1, 1.5, "3"])
def test_a_bad_seed_raises_np_randoms_error(bad):
    with pytest.raises(ValueError, match="non-negative integer"):
        seed_rows([0, bad])
