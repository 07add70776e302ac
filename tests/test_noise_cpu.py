"""CPU: the counter-based sampler noise (open_universe_amd/noise.py) -- the block function against its known answers,
position indexing, moments with bounds that follow from the sample size, the stream plan of the Python layer and the CLI's
`--noise` argument handling.  The device side is tests/test_gpu_noise.py."""
import math

import numpy as np
import pytest
import torch

from open_universe_amd import audio as A
from open_universe_amd import noise as N
from open_universe_amd.bin import enhance as cli

# Philox4x32-10, counter / key -> output (Random123's known-answer vectors)
KAT = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    got = N.philox4x32_10(np.array(_words(ctr), dtype=np.uint32), np.array(_words(key), dtype=np.uint32))
    assert [int(v) for v in got] == _words(out)


def test_philox_is_vectorised_over_counters():
    ctr = np.array([_words(k[0]) for k in KAT], dtype=np.uint32)
    key = np.array([_words(k[1]) for k in KAT], dtype=np.uint32)
    got = N.philox4x32_10(ctr, key)
    assert got.shape == (3, 4) and [[int(v) for v in r] for r in got] == [_words(k[2]) for k in KAT]


@pytest.mark.parametrize("t0", [0, 1, 2, 3, 4, 7, 1001, (1 << 32) - 3, (1 << 32) + 5, (1 << 40) + 2, (1 << 49) + 1])
def test_position_indexing(t0):
    """reference(.., t0, n) is the slice [t0 : t0 + n] of the row that starts at 0 -- here of the row that starts a little in
    front of t0 (a row from 0 to 2^40 cannot be held), and for small t0 of the row from 0 itself."""
    seed, stream, draw, n = 0x1234567890ABCDEF, (7 << 16) | 1, 3, 203
    a = N.reference(seed, stream, draw, t0, n)
    base = max(0, t0 - 9)
    whole = N.reference(seed, stream, draw, base, t0 - base + n)
    assert a.shape == (n,) and np.array_equal(a, whole[t0 - base:])
    if t0 < 5000:
        assert np.array_equal(a, N.reference(seed, stream, draw, 0, t0 + n)[t0:])
    # pieces tile
    assert np.array_equal(a, np.concatenate([N.reference(seed, stream, draw, t0, 5), N.reference(seed, stream, draw, t0 + 5, n - 5)]))


def test_every_argument_changes_the_block():
    base = dict(seed=11, stream=5, draw=2, t0=64, n=4)
    z = N.reference(**base)
    for k, v in (("seed", 12), ("seed", 11 + (1 << 32)), ("stream", 6), ("stream", 5 + (1 << 32)), ("stream", 5 + (1 << 48)),
                 ("draw", 3), ("t0", 68), ("t0", 64 + (1 << 34))):
        other = N.reference(**dict(base, **{k: v}))
        assert not np.any(other == z), (k, v)
    assert np.array_equal(z, N.reference(**base))


def test_moments():
    """2^22 values: |mean| < 5 / sqrt(N), |var - 1| < 5 sqrt(2 / N), correlation between two streams and between lag-1
    neighbours < 5 / sqrt(N) (five standard errors each); all finite and inside the 24-bit uniform's range."""
    n = 1 << 22
    a = N.reference(20240917, (3 << 16), 1, 0, n)
    b = N.reference(20240917, (4 << 16), 1, 0, n)
    assert a.dtype == np.float64 and np.isfinite(a).all() and np.isfinite(b).all()
    zmax = math.sqrt(2 * 25 * math.log(2))
    assert np.abs(a).max() <= zmax and np.abs(b).max() <= zmax
    se = 1.0 / math.sqrt(n)
    for z in (a, b):
        print(f"mean {z.mean():+.2e} (bound {5 * se:.2e})  var - 1 {z.var() - 1:+.2e} (bound {5 * math.sqrt(2.0 / n):.2e})")
        assert abs(z.mean()) < 5 * se
        assert abs(z.var() - 1.0) < 5 * math.sqrt(2.0 / n)
    corr = lambda x, y: float(np.mean((x - x.mean()) * (y - y.mean())) / (x.std() * y.std()))  # noqa: E731
    c_streams, c_lag = corr(a, b), corr(a[:-1], a[1:])
    c_draws = corr(a, N.reference(20240917, (3 << 16), 2, 0, n))
    print(f"corr streams {c_streams:+.2e}  lag-1 {c_lag:+.2e}  draws {c_draws:+.2e} (bound {5 * se:.2e})")
    assert abs(c_streams) < 5 * se and abs(c_lag) < 5 * se and abs(c_draws) < 5 * se


def test_reference_refuses_out_of_range():
    for kw in (dict(seed=-1), dict(seed=1 << 64), dict(stream=1 << 64), dict(draw=1 << 16), dict(draw=-1), dict(t0=-1),
               dict(t0=(1 << 50) - 3)):
        with pytest.raises(ValueError):
            N.reference(**dict(dict(seed=1, stream=0, draw=0, t0=0, n=8), **kw))
    assert N.reference(1, 0, 0, 5, 0).shape == (0,)


def test_counter_noise_streams():
    g = N.CounterNoise(7, stream=3)
    assert g.stream_ids(1) == [3 << 16] and g.stream_ids(3) == [(3 << 16) | c for c in range(3)]
    assert g.at(2) == N.CounterNoise(7, 5) and g.at(0) == g and hash(g.at(0)) == hash(g)
    # ensemble members get streams of their own, member-major like the replication in `enhance`
    ids = g.stream_ids(2, ensemble=3)
    assert ids == [(3 << 16) | c | (e << 48) for e in range(3) for c in range(2)] and len(set(ids)) == 6
    # no two (utterance, channel, member) triples share an id
    seen = set()
    for u in (0, 1, 2, (1 << 32) - 1):
        for v in N.CounterNoise(7, u).stream_ids(4, ensemble=5):
            assert 0 <= v < 1 << 64 and v not in seen
            seen.add(v)
    with pytest.raises(AttributeError):
        g.seed = 9
    for bad in (dict(seed=-1), dict(seed=1 << 64), dict(seed=1, stream=-1), dict(seed=1, stream=1 << 32)):
        with pytest.raises(ValueError):
            N.CounterNoise(**bad)
    with pytest.raises(ValueError):
        g.stream_ids(0)
    assert N.is_counter(g) and not N.is_counter(torch.Generator()) and not N.is_counter(None)


def test_enhance_many_stream_plan():
    """One shared source: entry i is utterance stream + i; one per entry: taken as given; channel c -> (utterance << 16) | c."""
    from open_universe_amd.universe import Universe

    plan = Universe._counter_plan
    assert plan(None, [1, 2]) is None and plan(torch.Generator(), [1]) is None
    assert plan([torch.Generator(), torch.Generator()], [1, 1]) is None
    seed, ids = plan(N.CounterNoise(9, 4), [1, 2, 1])
    assert seed == 9 and ids == [4 << 16, 5 << 16, (5 << 16) | 1, 6 << 16]
    seed, ids = plan([N.CounterNoise(9, 40), N.CounterNoise(9, 2)], [2, 1])
    assert ids == [40 << 16, (40 << 16) | 1, 2 << 16]
    with pytest.raises(ValueError, match="mix"):
        plan([N.CounterNoise(9, 0), torch.Generator()], [1, 1])
    with pytest.raises(ValueError, match="seed"):
        plan([N.CounterNoise(9, 0), N.CounterNoise(8, 1)], [1, 1])
    with pytest.raises(ValueError, match="same noise"):
        plan([N.CounterNoise(9, 3), N.CounterNoise(9, 3)], [1, 1])
    with pytest.raises(ValueError):
        plan([N.CounterNoise(9, 3)], [1, 1])


def test_sharded_noise_sources():
    from open_universe_amd import distributed as D

    assert D.utterance_noise("cpu", 5, 7, "counter") == N.CounterNoise(5, 7)
    g = D.utterance_noise("cpu", 5, 7, "generator")
    assert isinstance(g, torch.Generator) and g.initial_seed() == 12
    with pytest.raises(ValueError):
        D.utterance_noise("cpu", 5, 7, "philox")


# ---- CLI -------------------------------------------------------------------------------------------------------------------
class _Fake:
    """enhance(x) = x + 1e-3 * (utterance index + 1), recorded with the source it was handed."""
    fs = 16000
    device = "cpu"
    tot_ds = 1

    class _KW(dict):
        pass

    diff_kwargs = _KW(n_steps=8, epsilon=1.3)

    def __init__(self):
        self.seen, self.batches, self.long = [], [], []

    def enhance(self, mix, n_steps: int = None, epsilon: float = None, rng: torch.Generator = None, keep_rms: bool = False,
                target: torch.Tensor = None) -> torch.Tensor:
        self.seen.append(rng)
        return mix

    def enhance_many(self, sigs, rngs, pad_batch=False, **kw):
        self.batches.append(list(rngs))
        self.seen += list(rngs)
        return list(sigs)

    def enhance_long(self, mix, segment_s=8.0, overlap_s=1.0, rng=None, **kw):
        self.long.append(rng)
        self.seen.append(rng)
        return mix

    def advance_generator_like_enhance(self, *a, **k):
        raise AssertionError("counter mode must not re-draw any file's noise")


def _files(tmp_path, lens):
    src = tmp_path / "in"
    src.mkdir()
    for i, n in enumerate(lens):
        A.save(src / f"f{i}.wav", torch.zeros(1, n), 16000)
    return src


def test_cli_noise_flag_parses_and_defaults():
    p = cli.build_parser()
    assert p.parse_args(["a", "b"]).noise == "generator"
    assert p.parse_args(["a", "b", "--noise", "counter"]).noise == "counter"
    a = p.parse_args(["a", "b", "--noise", "counter", "--batch-size", "4"])
    assert a.noise == "counter" and a.batch_size == 4
    a = p.parse_args(["a", "b", "--noise", "counter", "--segment-seconds", "8"])
    cli.check_segment_args(a, {})
    cli.check_noise_args(a, {})
    with pytest.raises(SystemExit):
        p.parse_args(["a", "b", "--noise", "philox"])


def test_cli_noise_counter_refusals():
    p = cli.build_parser()
    a = p.parse_args(["a", "b", "--noise", "counter"])
    with pytest.raises(ValueError, match="target"):
        cli.check_noise_args(a, {"target": torch.zeros(1)})
    with pytest.raises(ValueError, match="per-file-seed"):
        cli.check_noise_args(p.parse_args(["a", "b", "--noise", "counter", "--per-file-seed"]), {})
    with pytest.raises(ValueError, match="seed"):
        cli.check_noise_args(p.parse_args(["a", "b", "--noise", "counter", "--seed", "-4"]), {})
    # generator mode: nothing to refuse (today's behaviour)
    cli.check_noise_args(p.parse_args(["a", "b", "--per-file-seed"]), {"target": torch.zeros(1)})
    # --pad-batch keeps refusing what it refuses today
    with pytest.raises(ValueError, match="pad-batch"):
        cli.check_segment_args(p.parse_args(["a", "b", "--noise", "counter", "--segment-seconds", "8", "--pad-batch"]), {})


def test_cli_stream_plan_is_the_file_index(tmp_path, monkeypatch):
    """File k of the sorted list is stream k of --seed: in the serial loop, batched and length-sorted, segmented, and on every
    rank of a sharded run -- without --per-file-seed and without a second draw."""
    assert N.plan_streams(3, 5) == {k: N.CounterNoise(5, k) for k in range(3)}
    assert N.plan_streams(9, 5, [7, 2]) == {7: N.CounterNoise(5, 7), 2: N.CounterNoise(5, 2)}
    lens = [900, 200, 800, 300, 700, 100, 600]
    src = _files(tmp_path, lens)
    want = [N.CounterNoise(21, k) for k in range(len(lens))]
    m = _Fake()
    cli.main([str(src), str(tmp_path / "o1"), "--seed", "21", "--noise", "counter"], model=m)
    assert m.seen == want
    m = _Fake()
    cli.main([str(src), str(tmp_path / "o2"), "--seed", "21", "--noise", "counter", "--batch-size", "2", "--batch-window", "4"],
             model=m)
    assert sorted(m.seen, key=lambda g: g.stream) == want
    # window 1 = files 0..3 sorted by length: (0, 2), (3, 1); window 2 = files 4..6: (4, 6), (5)
    assert [[g.stream for g in b] for b in m.batches] == [[0, 2], [3, 1], [4, 6], [5]]
    m = _Fake()
    cli.main([str(src), str(tmp_path / "o3"), "--seed", "21", "--noise", "counter", "--segment-seconds", "0.03", "--segment-overlap", "0.01"],
             model=m)
    assert m.seen == want
    # files longer than 0.03 s = 480 samples went through enhance_long with the same source
    assert m.long == [want[k] for k, n in enumerate(lens) if n > 480]
    # sharded: every rank hands file k the source of file k (nothing is forced, nothing depends on the shard)
    seen = {}
    monkeypatch.setenv("WORLD_SIZE", "3")
    for rank in range(3):
        monkeypatch.setenv("RANK", str(rank))
        m = _Fake()
        done = cli.main([str(src), str(tmp_path / f"r{rank}"), "--seed", "21", "--noise", "counter"], model=m)
        for p, g in zip(done, m.seen):
            seen[int(p.stem[1:])] = g
    assert [seen[k] for k in range(len(lens))] == want


def test_cli_generator_mode_is_unchanged(tmp_path):
    """--noise generator (the default): the shared generator of the serial loop, as before."""
    src = _files(tmp_path, [300, 200])
    for extra in ([], ["--noise", "generator"]):
        m = _Fake()
        cli.main([str(src), str(tmp_path / "o"), "--seed", "7"] + extra, model=m)
        assert all(isinstance(g, torch.Generator) and g.initial_seed() == 7 for g in m.seen) and m.seen[0] is m.seen[1]
