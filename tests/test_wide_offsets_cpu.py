"""Offsets past 4 GiB without a GPU: the planner of tests/wide_offsets.py held to its own rules, each asserted from the arrays it returns, and the library's host
rules (api.plan_placed, api.pcm_placed_offset, api.dec_plan_packed_lenient, api.plan_ingest, api.plan_packed) held at those numbers to the header's rule
restated here in Python integers, which do not wrap."""
import numpy as np
import pytest

import wide_offsets as wo

S = 6
FMT = {1: 0x84, 2: 16, 3: 0x82, 4: 0x80}             # a sample type of each element size: mu-law, int16, packed 24-bit LE, float32
IL = 0x100
ARENAS = [pytest.param(wo.ARENA, id="full"), pytest.param(wo.ARENA_REDUCED, id="reduced")]


def _api():
    from audio_codec_amd import api
    return api


def _ok(e, fe, cap):
    """the header's rule for a placed frame, restated: it lies inside [0, capacity)"""
    return 0 <= int(e) and int(e) + fe <= cap


def _ranges(offs, eb, fe):
    return [(int(e) * eb, (int(e) + fe) * eb) for e in np.asarray(offs).reshape(-1)]


def _hit(a, b):
    return a[0] < b[1] and b[0] < a[1]


def _in_class(cls, e, bd, eb, fe):
    """the position classes, restated as properties of the byte ranges"""
    first = -(-bd // eb)                                                  # first element at or above bd
    aligned = lambda x: (x * eb) % 16 == 0 and x >= first and not any((y * eb) % 16 == 0 for y in range(first, x))
    if cls == 0:
        return (e + fe) * eb <= bd < (e + fe + 1) * eb
    if cls == 1:
        return (e + fe // 2) * eb <= bd < (e + fe // 2 + 1) * eb and e * eb < bd < (e + fe) * eb
    if cls == 2:
        return (e + 1) * eb <= bd < (e + 2) * eb
    return aligned(e) if cls == 3 else aligned(e - 1)


def _check_plan(offs, cap, aliases, eb, fe_of, arena, T):
    """every rule of the planner, from what it returned; fe_of(k, s, t) -> the frame's elements"""
    bds = wo.bounds(arena)
    assert len(bds) == (4 if arena == wo.ARENA else 2) and offs.shape == (5, S, T) and offs.dtype == np.int64 and cap == arena // eb
    for k in range(5):
        frames = {(s, t): (int(offs[k, s, t]) * eb, (int(offs[k, s, t]) + fe_of(k, s, t)) * eb) for s in range(S) for t in range(T)}
        # valid, inside the arena with its guards
        for (s, t), (lo, hi) in frames.items():
            assert _ok(offs[k, s, t], fe_of(k, s, t), cap) and lo >= wo.GUARD and hi + wo.GUARD <= arena
        # every boundary in class k, on one frame each
        edge = {}
        for bd in bds:
            at = [st for st in frames if _in_class(k, int(offs[k][st]), bd, eb, fe_of(k, *st))]
            assert len(at) == 1, (k, bd, at)
            edge[at[0]] = bd
        # no two frames overlap, and no guard overlaps a frame
        order = sorted(frames.values())
        for a, b in zip(order[:-1], order[1:]):
            assert b[0] - a[1] >= wo.GUARD, (k, a, b)
        # the kept aliases: inside the arena, not the true range, narrowed as stated, clear of every frame and guard; every alias that is not kept is
        # outside the arena, the true range, or another boundary frame of the call
        guarded = [(lo - wo.GUARD, hi + wo.GUARD) for lo, hi in order]
        n_kept = 0
        for (s, t), (lo, hi) in frames.items():
            e, kept = int(offs[k, s, t]), aliases[k][s][t]
            starts = {(e % 2 ** 32) * eb, (e % 2 ** 31) * eb, (e * eb) % 2 ** 32, (e * eb) % 2 ** 31}
            for a in kept:
                assert a[0] in starts and a[1] - a[0] == hi - lo and a[1] <= arena and a[0] != lo
                assert not any(_hit(a, g) for g in guarded), (k, s, t, a)
            n_kept += len(kept)
            for a0 in starts - {a[0] for a in kept}:
                a = (a0, a0 + hi - lo)
                assert a[1] > arena or a0 == lo or ((s, t) in edge and any(_hit(a, frames[o]) for o in edge if o != (s, t))), (k, s, t, a)
        assert n_kept >= S                                                # every far frame has some
        # low and deep frames: both kinds, deep ones strictly between boundaries, both alignments among them
        rest = [st for st in frames if st not in edge]
        low = [st for st in rest if frames[st][1] < 2 ** 31]
        deep = [st for st in rest if frames[st][0] > 2 ** 31]
        assert len(low) + len(deep) == len(rest) and len(low) >= S and len(deep) >= S
        for st in deep:
            assert not any(frames[st][0] - wo.GUARD <= bd <= frames[st][1] + wo.GUARD for bd in bds)
        assert any(frames[st][0] % 16 == 0 for st in deep) and any(int(offs[k][st]) % 2 == 1 and frames[st][0] % 16 for st in deep)
        # a step of more than 2^32 bytes in each direction, in every stream
        for s in range(S):
            step = [frames[(s, t + 1)][0] - frames[(s, t)][0] for t in range(T - 1)]
            assert max(step) > 2 ** 32 and min(step) < -2 ** 32, (k, s)


@pytest.mark.parametrize("arena", ARENAS)
@pytest.mark.parametrize("T", [4, 12])
@pytest.mark.parametrize("N", [40, 160, 240, 480, 960])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("eb", [1, 2, 3, 4])
def test_planner_keeps_its_rules(eb, channels, N, T, arena):
    fe = channels * N
    offs, cap, aliases = wo.plan(eb, channels, N, S, T, arena=arena, seed=eb * 1000 + N + channels)
    _check_plan(offs, cap, aliases, eb, lambda k, s, t: fe, arena, T)
    again = wo.plan(eb, channels, N, S, T, arena=arena, seed=eb * 1000 + N + channels)
    assert np.array_equal(offs, again[0]) and aliases == again[2]       # the same seed, the same plan


@pytest.mark.parametrize("arena", ARENAS)
@pytest.mark.parametrize("T", [4, 12])
def test_planner_for_packed_frames(T, arena):
    sizes = np.random.default_rng(T).choice([40, 80, 128, 130, 161, 400], size=(5, S, T))
    offs, cap, aliases = wo.plan_bytes(sizes, arena=arena, seed=3)
    assert cap == arena
    _check_plan(offs, cap, aliases, 1, lambda k, s, t: int(sizes[k, s, t]), arena, T)


def test_boundaries_are_the_element_offsets_they_stand_for():
    """element offset 2^31 of every element size and 2^32 of one and two bytes are among the byte boundaries (three bytes: to within an element)"""
    for eb in (1, 2, 4):
        assert 2 ** 31 * eb in wo.BOUNDS
    assert any(abs(2 ** 31 * 3 - b) < 3 for b in (3 * 2 ** 31,)) and 3 * 2 ** 31 in wo.BOUNDS
    assert 2 ** 32 * 1 in wo.BOUNDS and 2 ** 32 * 2 in wo.BOUNDS
    assert wo.ARENA == 2 ** 33 + 2 ** 28 and wo.ARENA_REDUCED == 2 ** 32 + 2 ** 28


def test_alias_invalid_is_out_of_range_in_64_bits_and_in_range_in_32():
    cap = 5000
    v = np.array([[0, 17], [960, 4000]], np.int64)
    out = wo.alias_invalid(v, cap)
    assert out.shape == (5, 2, 2) and out.dtype == np.int64
    for row in out:
        for a, b in zip(row.reshape(-1), v.reshape(-1)):
            assert not 0 <= int(a) < cap
            assert int(a) % 2 ** 31 == int(b)                            # narrowed to 31 or 32 bits it is the valid offset again


# ---- the host rules at these numbers ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arena", ARENAS)
@pytest.mark.parametrize("channels,N", [(1, 480), (2, 480), (2, 160), (1, 960), (1, 240)])
@pytest.mark.parametrize("eb", [1, 2, 3, 4])
def test_plan_placed_and_placed_offset_past_4g(eb, channels, N, arena):
    api = _api()
    fe = channels * N
    offs, cap, _ = wo.plan(eb, channels, N, S, 4, arena=arena, seed=eb + N)
    assert not api.plan_placed(FMT[eb], channels, N, offs, cap).any()
    # the capacity edge, at every capacity a frame of the plan ends on: valid there, invalid one element further
    for e in offs.reshape(-1)[::7]:
        e = int(e)
        got = api.plan_placed(FMT[eb], channels, N, np.array([e, e + 1, e - 1], np.int64), e + fe)
        assert got.tolist() == [0, 1, 0] and [not _ok(x, fe, e + fe) for x in (e, e + 1, e - 1)] == [False, True, False]
    # one sample's element index: channel after channel with no layout bit, sample by sample interleaved
    for e in offs.reshape(-1)[::5]:
        e = int(e)
        for ch, i in ((0, 0), (channels - 1, N - 1), (channels - 1, 0), (0, N // 2)):
            assert api.pcm_placed_offset(FMT[eb], channels, N, e, ch, i) == e + ch * N + i
            assert api.pcm_placed_offset(FMT[eb] | IL, channels, N, e, ch, i) == e + i * channels + ch
    # out of range in 64 bits, in range in 32: refused, against a small capacity
    small = 64 * fe
    valid = (np.arange(24, dtype=np.int64) * fe + 3).reshape(6, 4)[:, :3]
    bad = wo.alias_invalid(valid, small)
    assert api.plan_placed(FMT[eb], channels, N, bad, small).all() and not api.plan_placed(FMT[eb], channels, N, valid, small).any()
    assert all(not _ok(x, fe, small) for x in bad.reshape(-1))
    for x in bad[2].reshape(-1):                                          # the negative ones have no sample address either
        assert api.pcm_placed_offset(FMT[eb], channels, N, int(x), 0, 0) == -1


@pytest.mark.parametrize("arena", ARENAS)
@pytest.mark.parametrize("channels,size", [(1, 80), (1, 130), (2, 160)])
def test_dec_plan_packed_and_ingest_past_4g(channels, size, arena):
    """frames of one size at the planner's byte offsets: none invalid against the arena as capacity; the capacity edge; ingest carries all 64 bits"""
    api = _api()
    T = 4
    sizes = np.full((5, S, T), size, np.int64)
    offs, cap, _ = wo.plan_bytes(sizes, arena=arena, seed=size)
    start = np.full(S, size, np.int32)
    nb = np.full((S, T), size, np.int32)
    for k in range(5):
        rc, eff, lost, inv, end, mx = api.dec_plan_packed_lenient(48000, channels, 10.0, 0, start, nb, offs[k], cap, size)
        assert rc == 0 and not inv.any() and not lost.any() and (eff == size).all()
        edge = int(offs[k].max()) + size                                   # the capacity that ends on the highest frame's last byte, and one byte less
        assert not api.dec_plan_packed_lenient(48000, channels, 10.0, 0, start, nb, offs[k], edge, size)[3].any()
        inv = api.dec_plan_packed_lenient(48000, channels, 10.0, 0, start, nb, offs[k], edge - 1, size)[3]
        assert np.array_equal(inv != 0, offs[k] + size > edge - 1) and inv.sum() == 1
        # ingest: one item per cell in a shuffled list, sequence numbers that wrap
        order = np.random.default_rng(k).permutation(S * T)
        base = np.array([65534, 3, 65535, 0, 40000, 65533])
        stream = np.repeat(np.arange(S), T)[order]
        seq = ((base[:, None] + np.arange(T)[None, :]) & 0xFFFF).reshape(-1)[order]
        out = api.plan_ingest(S, channels, stream, seq, offs[k].reshape(-1)[order], nb.reshape(-1)[order], base, T)
        assert out["offsets"].dtype == np.int64 and np.array_equal(out["offsets"], offs[k]), "ingest did not carry an offset's 64 bits"
        assert np.array_equal(out["num_bytes"], nb) and (out["counts"] == T).all()
    # out of range in 64 bits, in range in 32: every such frame invalid; ingest still carries it unchanged, for the decoder to refuse
    small = S * T * (size + 5) + 9
    valid = (np.arange(S * T, dtype=np.int64) * (size + 5) + 1).reshape(S, T)
    assert not api.dec_plan_packed_lenient(48000, channels, 10.0, 0, start, nb, valid, small, size)[3].any()
    for bad in wo.alias_invalid(valid, small):
        rc, eff, lost, inv, end, mx = api.dec_plan_packed_lenient(48000, channels, 10.0, 0, start, nb, bad, small, size)
        assert rc == 0 and inv.all()
        assert all(not (0 <= int(x) and int(x) + size <= small) for x in bad.reshape(-1))
        base = np.zeros(S, np.int64)
        out = api.plan_ingest(S, channels, np.repeat(np.arange(S), T), np.tile(np.arange(T), S), bad.reshape(-1), nb.reshape(-1), base, T)
        assert np.array_equal(out["offsets"], bad)


def test_plan_packed_capacity_is_64_bits():
    """capacity 2^32 + 10 and capacity 10: a capacity narrowed to 32 bits would make the two alike"""
    api = _api()
    sizes = np.random.default_rng(5).choice([3, 4, 40, 80, 161], size=(S, 12)).astype(np.int32)
    sizes[0, 0], sizes[0, 1] = 4, 6                                       # the first frame fits 10 bytes, the second ends on them, the third does not fit
    for order in (0, 1):
        rc, offs, total, big = api.plan_packed(sizes, order, 2 ** 32 + 10)
        rc2, offs2, total2, small = api.plan_packed(sizes, order, 10)
        assert rc == 0 and rc2 == 0 and np.array_equal(offs, offs2) and total == total2 == int(sizes.sum())
        fits = np.array([[int(offs[s, t]) + int(sizes[s, t]) <= 10 for t in range(12)] for s in range(S)])
        assert not big.any(), "a frame below 2^32 + 10 bytes was cut"
        assert np.array_equal(small, np.where(fits, 0, api.ENC_FL_PACK_CAP).astype(np.uint8)) and fits.sum() >= 1 and not fits.all()
        assert np.array_equal(big != small, ~fits)
