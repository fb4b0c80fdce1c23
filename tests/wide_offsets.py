"""Offsets past 4 GiB (test infrastructure, a plain helper beside size_sweep.py and hostile_frames.py; pure numpy, no library call).

The batch interface takes 64-bit offsets - placed PCM in elements (lc3plus_{enc,dec}_batch_set_pcm_placement), packed frames and probe items in bytes - and
the other tests only ever use in-range offsets of a few megabytes.  This helper plans the frames of a call inside ONE arena of ARENA bytes addressed from its
base: the pointer handed to the library is the arena base, so element e of a type of eb bytes is byte e * eb.  tests/test_wide_offsets_cpu.py asserts every rule
below from the returned arrays and holds the host rules to them; tests/test_gpu_wide_offsets.py runs the kernels on the plans.

Boundaries (bytes): 2^31, 2^32, 3 * 2^31, 2^33 - the byte offsets 2^31, 2^32, 2^33 of every type, element offset 2^31 of eb = 1, 2, 3 (to within an element), 4
and element offset 2^32 of eb = 1, 2.  The reduced arena keeps the first two.

Position classes of a frame of fe elements at boundary Bd, with below = Bd // eb the number of elements that lie wholly below Bd:
  0  the frame ends at the last element wholly below Bd                      start = below - fe
  1  it straddles Bd in its middle (stereo, no layout bit: channel 0 below)   start = below - fe // 2
  2  exactly one element lies below Bd                                        start = below - 1
  3  it starts at the first element at or above Bd whose byte address is 16-byte aligned (the wide load / store form; with eb = 3 that is the first element
     index that is a multiple of 16, at most 47 bytes above Bd: Bd itself is no multiple of 3)
  4  one element further than class 3 (the element-by-element form)

plan(): call k holds class k at every boundary, one frame per boundary (the classes of one boundary overlap one another, so they are never in one call).  Every
stream has, in every call, three consecutive frames low, far, low with far - low > 2^32 bytes: a step of more than 2^32 in each direction.  The remaining frames
are drawn half from the low offsets (below 2^31 bytes), half from the deep ones (strictly between boundaries, or between the last boundary and the end of the
arena), the deep ones by turns 16-byte aligned and at an odd element.  Within a call no two frames overlap, and GUARD bytes on each side of every frame overlap
no frame and lie inside the arena.

Aliases of a frame at element e are the byte ranges it would occupy if the arithmetic were narrowed, starting at (e mod 2^32) * eb, (e mod 2^31) * eb,
(e * eb) mod 2^32 and (e * eb) mod 2^31; each is kept where it lies inside the arena and differs from the true range.  No kept alias overlaps any frame or guard
of its call: the low and deep frames are redrawn until that holds.  One exception is inherent in the construction and not a choice: the boundaries are 2^31
bytes apart, so the alias of the boundary frame at 2^32 + d IS the boundary frame of the same class at 2^31 + d.  Such an alias - one that overlaps another
boundary frame of the call - is not kept; a narrowed access there does not go unseen, since it reads or overwrites a frame whose content is compared."""
import numpy as np

ARENA = 2 ** 33 + 2 ** 28
ARENA_REDUCED = 2 ** 32 + 2 ** 28
BOUNDS = (2 ** 31, 2 ** 32, 3 * 2 ** 31, 2 ** 33)
CLASSES = 5
GUARD = 256
LOW_END = 2 ** 31
STEP_LOW_END = 2 ** 27                       # the low frames of the low, far, low triple lie below this ...
STEP_FAR_START = 2 ** 32 + 2 ** 27 + 2 ** 20  # ... and the far one at or above this: more than 2^32 apart
I64_MAX = 2 ** 63 - 1


def bounds(arena=ARENA):
    return tuple(b for b in BOUNDS if b < arena)


def class_start(cls, bd, eb, size):
    """first element of the frame of `size` elements in position class cls at boundary bd (bytes)"""
    below = bd // eb
    first = -(-bd // eb)
    while (first * eb) % 16:
        first += 1
    return {0: below - size, 1: below - size // 2, 2: below - 1, 3: first, 4: first + 1}[cls]


def alias_starts(e, eb):
    """the byte addresses a frame at element e would start at if an offset were narrowed to 32 or 31 bits, before or after the multiplication by eb"""
    return ((e % 2 ** 32) * eb, (e % 2 ** 31) * eb, (e * eb) % 2 ** 32, (e * eb) % 2 ** 31)


def frame_aliases(e, eb, size, arena):
    """kept alias byte ranges [(lo, hi)] of a frame of `size` elements at element e: inside the arena, different from the true range"""
    out = []
    for a in alias_starts(e, eb):
        r = (a, a + size * eb)
        if r[1] <= arena and a != e * eb and r not in out:
            out.append(r)
    return out


def _overlap(a, b):
    return a[0] < b[1] and b[0] < a[1]


def _deep_regions(arena):
    edges = bounds(arena) + (arena,)
    return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]


def _slots(S, T, k, nb):
    """who is what in call k: triple[s] = first slot of the low, far, low run of stream s; edge[(s, t)] = boundary index"""
    assert T >= 4 and nb <= S * (T - 3)
    triple = [(s + k) % (T - 2) for s in range(S)]
    edge = {}
    for b in range(nb):
        s = (b + k) % S
        free = [t for t in range(T) if not triple[s] <= t < triple[s] + 3]
        t = free[(k + s + b // S) % len(free)]
        assert (s, t) not in edge
        edge[(s, t)] = b
    return triple, edge


def _plan(eb, sizes, calls, arena, seed):
    """sizes [calls, S, T] in elements -> (offsets [calls, S, T] int64, aliases[k][s][t] = [(lo, hi) bytes])"""
    sizes = np.asarray(sizes, np.int64)
    K, S, T = sizes.shape
    assert K == calls <= CLASSES and eb in (1, 2, 3, 4)
    bds = bounds(arena)
    deep = _deep_regions(arena)
    far = [(max(lo, STEP_FAR_START), hi) for lo, hi in deep if hi > STEP_FAR_START + 2 ** 20]
    rng = np.random.default_rng(seed)
    offsets = np.zeros((K, S, T), np.int64)
    aliases = []

    def draw(lo, hi, size, how):
        """an element offset whose frame and guards lie inside bytes (lo, hi): how = 'any', 'aligned' (byte address a multiple of 16) or 'odd' (element)"""
        e_lo, e_hi = -(-(lo + GUARD + 1) // eb), (hi - GUARD - 1) // eb - size
        e = int(rng.integers(e_lo, e_hi))
        if how == "aligned":
            e -= e % 16
            if e < e_lo:
                e += 16
        elif how == "odd":
            e |= 1
            if e > e_hi:
                e -= 2
        assert e_lo <= e <= e_hi
        return e

    for k in range(K):
        triple, edge = _slots(S, T, k, len(bds))
        fixed = {st: class_start(k, bds[b], eb, int(sizes[k, st[0], st[1]])) for st, b in edge.items()}
        for attempt in range(1000):
            off = {}
            ndeep = 0
            for s in range(S):
                for t in range(T):
                    size = int(sizes[k, s, t])
                    if (s, t) in fixed:
                        off[(s, t)] = fixed[(s, t)]
                    elif t in (triple[s], triple[s] + 2):
                        off[(s, t)] = draw(0, STEP_LOW_END, size, "any")
                    elif t == triple[s] + 1:
                        lo, hi = far[int(rng.integers(len(far)))]
                        off[(s, t)] = draw(lo, hi, size, "aligned" if s % 2 == 0 else "odd")
                    elif (s + t + k) % 2 == 0:
                        off[(s, t)] = draw(0, LOW_END, size, "any")
                    else:
                        lo, hi = deep[int(rng.integers(len(deep)))]
                        off[(s, t)] = draw(lo, hi, size, "aligned" if ndeep % 2 == 0 else "odd")
                        ndeep += 1
            rng_of = {st: (e * eb, (e + int(sizes[k, st[0], st[1]])) * eb) for st, e in off.items()}
            order = sorted(rng_of.values())
            if any(b[0] - a[1] < GUARD for a, b in zip(order[:-1], order[1:])) or order[0][0] < GUARD or order[-1][1] + GUARD > arena:
                continue
            guarded = [(lo - GUARD, hi + GUARD) for lo, hi in order]
            al, clash = {}, False
            for st, e in off.items():
                kept = []
                for a in frame_aliases(e, eb, int(sizes[k, st[0], st[1]]), arena):
                    if st in fixed and any(_overlap(a, rng_of[o]) for o in fixed if o != st):
                        continue                                        # the inherent one: another boundary frame of the call (module docstring)
                    if any(_overlap(a, g) for g in guarded):
                        clash = True
                    kept.append(a)
                al[st] = kept
            if not clash:
                break
        else:
            raise RuntimeError("no plan found for call %d" % k)
        for (s, t), e in off.items():
            offsets[k, s, t] = e
        aliases.append([[al[(s, t)] for t in range(T)] for s in range(S)])
    return offsets, aliases


def plan(eb, channels, N, S, T, calls=CLASSES, arena=ARENA, seed=0):
    """placed PCM frames of channels * N elements of eb bytes -> (offsets [calls, S, T] int64 in elements, capacity in elements, aliases[k][s][t] = [(lo, hi)]
    byte ranges)"""
    offsets, aliases = _plan(eb, np.full((calls, S, T), channels * N, np.int64), calls, arena, seed)
    return offsets, arena // eb, aliases


def plan_bytes(sizes, calls=CLASSES, arena=ARENA, seed=0):
    """the same construction for the byte offsets of packed frames: eb = 1 and sizes [calls, S, T] bytes, one per frame -> (offsets, capacity, aliases)"""
    offsets, aliases = _plan(1, sizes, calls, arena, seed)
    return offsets, arena, aliases


def edge_slots(S, T, k, arena=ARENA):
    """{(s, t): boundary index} of call k, and the first slot of each stream's low, far, low run"""
    triple, edge = _slots(S, T, k, len(bounds(arena)))
    return edge, triple


ALIAS_INVALID = ("+2^32", "+2^33", "-2^32", "+2^31", "|2^62")


def alias_invalid(valid_offsets, capacity):
    """offsets that are out of range in 64 bits but in range once truncated, for small arenas (capacity below 2^31): valid_offsets (any shape, each inside
    [0, capacity)) -> int64 [5, ...]: v + 2^32, v + 2^33, v - 2^32, v + 2^31 (which exceeds the capacity) and v | 2^62, in the order of ALIAS_INVALID"""
    v = np.asarray(valid_offsets, np.int64)
    assert 0 <= capacity < 2 ** 31 and (v >= 0).all() and (v < max(capacity, 1)).all()
    out = np.stack([v + 2 ** 32, v + 2 ** 33, v - 2 ** 32, v + 2 ** 31, v | (1 << 62)])
    assert ((out < 0) | (out > capacity)).all()
    return out
