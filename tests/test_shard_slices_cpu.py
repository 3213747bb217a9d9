"""The slice arithmetic of the sharded gradient exchange (trainer.split_slice / trainer.owned_range), exhaustively and without a
process group: worlds 1..16, every slice length around the granule multiples -- the all-tail branch (a slice shorter than one granule
of 256 * world elements) included, which no end-to-end run of the tiny model reaches below 17 ranks."""
from xlxmert_amd.trainer import owned_range, split_slice

CHUNK = 256
WORLDS = range(1, 17)
LOWS = (0, CHUNK, CHUNK * 7)


def lengths(world):
    """in 256-element chunks: 0 .. 3 granules in steps of one chunk -- which holds one chunk either side of every granule multiple,
    one granule minus a chunk (all tail) and exactly one granule; named again so that none of them depends on the range's end"""
    gran = world
    chunks = set(range(0, 3 * gran + 1))
    for m in range(0, 4):
        chunks.update(c for c in (m * gran - 1, m * gran, m * gran + 1) if c >= 0)
    chunks.update((gran - 1, gran))
    return sorted(c * CHUNK for c in chunks)


def test_split_slice_and_owned_range_partition_every_slice():
    n_all_tail = n_cases = 0
    for world in WORLDS:
        gran = CHUNK * world
        for n in lengths(world):
            for lo in LOWS:
                hi = lo + n
                segs = split_slice(lo, hi, world)
                n_cases += 1
                # the segments tile [lo, hi) in order: at most one "rs", then at most one "ar"
                assert [k for k, _, _ in segs] in ([], ["rs"], ["ar"], ["rs", "ar"]), (world, lo, n, segs)
                pos = lo
                for kind, a, b in segs:
                    assert a == pos and b > a, (world, lo, n, segs)
                    pos = b
                assert pos == hi, (world, lo, n, segs)
                assert (segs == []) == (n == 0)
                for kind, a, b in segs:
                    pieces = [owned_range(kind, a, b, r, world) for r in range(world)]
                    if kind == "ar":
                        assert b - a < gran, (world, lo, n, segs)                  # a tail is shorter than one granule
                        assert all(p == (a, b) for p in pieces)                    # ... and owned whole by every rank
                        continue
                    assert (b - a) % gran == 0, (world, lo, n, segs)
                    # the ranks' pieces: rank order, end to end, from a to b -- disjoint and complete -- equally long, and whole
                    # 256-element chunks at both ends (flags[a // 256:b // 256] of the sharded optimizer pass is exact)
                    pos = a
                    for pa, pb in pieces:
                        assert pa == pos and pb - pa == (b - a) // world > 0, (world, lo, n, pieces)
                        assert pa % CHUNK == 0 and pb % CHUNK == 0, (world, lo, n, pieces)
                        pos = pb
                    assert pos == b
                    assert len(set(pieces)) == world
                tail = sum(b - a for k, a, b in segs if k == "ar")
                assert tail == n % gran
                if 0 < n < gran:                                                    # the all-tail branch
                    assert segs == [("ar", lo, hi)]
                    n_all_tail += 1
                if n == gran:
                    assert segs == [("rs", lo, hi)]
                if world == 1 and n:
                    assert len(segs) == 1 and segs[0][1:] == (lo, hi)               # one segment covering everything
    assert n_all_tail >= 3 * 15 and n_cases > 16 * 3 * 20


def test_lengths_hold_the_named_cases():
    for world in WORLDS:
        ls, gran = lengths(world), CHUNK * world
        assert set(range(0, 3 * gran + 1, CHUNK)) <= set(ls)
        for m in (1, 2, 3):
            assert {m * gran - CHUNK, m * gran, m * gran + CHUNK} <= set(ls)
        assert gran - CHUNK in ls and gran in ls and 0 in ls and CHUNK in ls
