"""bench.py's own contract: a plain run prints the headline line only, ``--full`` adds the CPU
baseline and the steady-state stream, ``--dump-outputs`` writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

WORDS = 2000  # 5.8 MB of candidates: dumped whole


def _bench(*args, words=WORDS):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--words", str(words), *args]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _u64(halves):
    h = halves.astype(np.uint64)
    return h[:, 0::2] | (h[:, 1::2] << np.uint64(32))


def _oracle_digests(words):
    from hashcat_a5_table_generator_amd import synth
    from oracle import c_oracle as co
    tables, (data, offs) = synth.global_words("c3", 0, words, seed=0x5A5)
    return co.CTable([os.path.join(ROOT, "tests", "golden", "tables", t + ".table") for t in tables]
                     ).digest_batch(data, offs, 0, 0, 15)


def test_plain_run_dumps_its_outputs(tmp_path):
    """The plain line has the headline fields and neither extra leg; the dumped arrays are
    float32 / float64, the same in a second run, and agree with the C oracle: per-word
    {candidates, bytes, sum h, sum h^2} of every word, the byte offsets their prefix sum."""
    r = _bench("--dump-outputs", str(tmp_path / "a"))
    _bench("--dump-outputs", str(tmp_path / "b"))
    assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["unit"] == "candidates/s"
    assert r["higher_is_better"] is True and r["dtype"] == "u8" and r["value"] > 0
    assert r["cpu_baseline"] is None and r["steady_state"] is None
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["byte_off", "candidates", "chunk_off", "totals", "word_digest"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64_000_000
    for k, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy"))), k
    want = _oracle_digests(WORDS)
    w = a["word_digest"][:, 0].astype(np.int64)
    assert np.array_equal(w, np.arange(WORDS))
    assert np.array_equal(_u64(a["word_digest"][:, 1:]), want)
    tc, tb = int(want[:, 0].sum()), int(want[:, 1].sum())
    assert a["totals"].tolist() == [tc, tb, WORDS] and r["config"]["candidates_per_gpu_step"] == tc
    assert np.array_equal(a["byte_off"][:, 0], np.arange(WORDS + 1))
    assert np.array_equal(a["byte_off"][:, 1], np.concatenate([[0], np.cumsum(want[:, 1])]))
    assert a["chunk_off"].tolist() == [0] and len(a["candidates"]) == tb
    assert int((a["candidates"] == 10).sum()) == tc  # one "\n" per candidate


def test_dump_samples_a_large_output(tmp_path):
    """20000 words write 60 MB: the stream is dumped as 2048 chunks of 4 KiB at seeded offsets
    inside it, the digests cover every word's whole output all the same."""
    words = 20000
    _bench("--dump-outputs", str(tmp_path), words=words)
    a = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    want = _oracle_digests(words)
    tb = int(want[:, 1].sum())
    assert a["totals"].tolist() == [int(want[:, 0].sum()), tb, words]
    assert a["candidates"].dtype == np.float32 and a["candidates"].shape == (2048 * 4096,)
    off = a["chunk_off"].astype(np.int64)
    assert len(off) == 2048 and (np.diff(off) > 0).all() and (off % 4096 == 0).all() and off[0] >= 0 and off[-1] + 4096 <= tb
    assert np.array_equal(a["word_digest"][:, 0], np.arange(words))
    assert np.array_equal(_u64(a["word_digest"][:, 1:]), want)
    assert np.array_equal(a["byte_off"][:, 1], np.concatenate([[0], np.cumsum(want[:, 1])]))


def test_full_run_adds_cpu_baseline_and_steady_state():
    r = _bench("--full", "--cpu-sample-words", "2000")
    assert r["ms_per_step"] > 0 and r["steps"] == 2
    assert r["cpu_baseline"]["value"] > 0 and r["steady_state"]["value"] > 0
