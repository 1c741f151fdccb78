"""The small word stage of k_keyspace_thread as the host sizes it (no GPU): what the compiled
table leaves of a 32,000 B workgroup (25 LDS granules of 1280 B: five workgroups per CU), a
multiple of 16, offered from 2048 B up."""
import numpy as np
import pytest

from conftest import table_path

FIXED = 16384 + 64 + 32 + 8192 + 512  # open groups, scan sums, stage slack, unit log, record sizes


def _small(tables):
    from hashcat_a5_table_generator_amd import Context
    with Context(-1) as c:
        c.load_tables([table_path(t) for t in tables])
        return c.keyspace_small_stage()


def test_small_stage_sizes():
    one, two = _small(["czech"]), _small(["czech", "german"])
    for s in (one, two):
        assert s % 16 == 0 and 2048 <= s <= 32000 - FIXED
    assert two < one  # the larger table leaves less
    # the tiles of C3's synthetic list (256 words of <= 12 bytes, 9 on average) fit
    from hashcat_a5_table_generator_amd import synth
    _, (_, offs) = synth.config_words("c3", 100000)
    o = offs.astype(np.int64)
    t0 = np.arange(0, len(o) - 1, 256)
    assert int((o[np.minimum(t0 + 256, len(o) - 1)] - (o[t0] & ~15)).max()) <= two


def test_small_stage_needs_table():
    from hashcat_a5_table_generator_amd import A5xError, Context
    with Context(-1) as c:
        with pytest.raises(A5xError):
            c.keyspace_small_stage()
        with pytest.raises(A5xError):
            c.keyspace_stage()  # a host-only context runs no keyspace pass
