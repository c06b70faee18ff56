"""The premises of tests/test_gpu_compress_seams.py, held against the oracle's tokens on the CPU: the crafted inputs of
tests/compress_craft.py really put a lone match over every seam offset, really carry every parse phase over a seam, really hold tiles
whose last-32 transfer function is constant next to tiles where it is not -- so that the GPU comparison cannot pass on inputs that miss
the edge they were built for."""
import numpy as np
import pytest

import compress_craft as craft
from compress_craft import TILE, SEAMS, N0, N7, WINDOWS, fields

MODEL_WINDOWS = [(32, 10), (32, 5), (64, 10), (200, 10), (256, 10), (256, 5)]


def _token_at(pos, ln, ds, p):
    i = int(np.searchsorted(pos, p))
    return (int(ln[i]), int(ds[i])) if i < len(pos) and pos[i] == p else None


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_lone_matches_start_at_every_offset_and_cross_the_seam_by_every_amount(oracle, cw, mm):
    total = chance = 0
    starts, cross, far_seen = set(), set(), 0
    dists_in = set()
    for n, cases in craft.family_a(cw, mm).items():
        for lab, b in cases:
            f = fields(lab)
            S, o, L, d = f["S"], f["o"], f["L"], f["d"]
            p = S + o
            pos, ln, ds = craft.token_arrays(oracle, b, cw, mm)
            tok = _token_at(pos, ln, ds, p)
            if f["twin"]:
                assert tok is None or tok[0] == 0 or tok[1] != d, (lab, tok)            # no 3-byte match at that distance
                if f["far"]:
                    total += 1
                    if tok is not None and tok[1] == cw and tok[0] >= min(L, mm):
                        far_seen += 1
                    else:
                        assert tok is None or (0 < tok[0] and tok[1] < cw), (lab, tok)   # only a nearer chance match may win, here or
                                                                                         # just in front (its token then covers p)
                        chance += 1
                continue
            if d > cw:
                assert tok is None or tok[0] == 0 or tok[1] != d, (lab, tok)            # one byte outside the window
                continue
            total += 1
            if tok == (min(L, mm), d):
                starts.add(o)
                dists_in.add(d)
                if o < 0 and p + tok[0] > S:
                    cross.add(p + tok[0] - S)
            else:
                assert tok is None or (0 < tok[0] and tok[1] < d), (lab, tok)           # only a nearer chance match may win
                chance += 1
    assert chance <= total // 100, (chance, total)
    assert starts == set(craft.OFFSETS_A)
    assert cross >= set(range(1, mm)), sorted(cross)
    assert dists_in == {d for d in craft.distances_a(cw) if d <= cw}
    assert far_seen >= (8 if cw >= 64 else 1), far_seen
    assert sum(len(c) for c in craft.family_a(cw, mm).values()) <= 1000


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("cw,mm", [(32, 10), (20, 10), (64, 10), (256, 5)])
def test_neighbours_in_memory_offer_a_candidate_in_front_and_an_extension_behind(oracle, cw, mm):
    for lab, n, pitch, nb, mem in craft.family_b(cw, mm):
        ends = 0
        for k in range(nb):
            at = k * pitch
            pos, ln, ds = craft.token_arrays(oracle, mem[at:at + n], cw, mm)
            assert ln[0] == 0                                            # the block's first token is a literal
            assert int((pos + np.maximum(ln, 1)).max()) == n and ln[-1] == 0      # no token reaches n: the last byte is a literal
            m = np.nonzero(ln)[0]
            assert (ds[m] <= pos[m]).all()                               # no candidate in front of the block
            d, j = craft.b_fields(k + 1, cw)                             # the end of this block
            run = craft.b_run(k + 1)
            assert mem[at + n - run:at + n + 3] == bytes(mem[i - d] for i in range(at + n - run, at + n + 3))   # the bytes behind would extend
            last = m[-1]
            if ds[last] == d and pos[last] + ln[last] == n - 2 and ln[last] < mm:
                ends += 1                                                # a match cut by the end of the block, not by maxmatch
            if k:
                d, j = craft.b_fields(k, cw)                             # the front of this block
                assert d <= cw and (j < 4 or mem[at + 1:at + 4] == mem[at + 1 - d:at + 4 - d])   # position 1: a candidate in memory, in the window
                assert mem[at:at + j] == bytes(mem[i - d] for i in range(at, at + j))
        assert ends >= nb // 4, (lab, ends)


# ------------------------------------------------------------------------------------------------ C
def _seam_skips(oracle, b, cw, mm):
    pos, ln, _ = craft.token_arrays(oracle, b, cw, mm)
    return [int(s) for s in craft.entry_skips(pos, ln, [S for S in SEAMS + (3 * TILE,) if S < len(b)])]


@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_every_entry_skip_occurs_at_a_seam(oracle, cw, mm):
    seen = [set(), set()]
    plain = set()
    for n, cases in craft.family_c(cw, mm).items():
        for lab, b in cases:
            sk = _seam_skips(oracle, b, cw, mm)
            seen[0].add(sk[0])
            seen[1].add(sk[1])
            if not fields(lab)["defect"]:
                plain.update(sk[:2])
            if fields(lab)["per"] == cw + 1:
                assert craft.token_arrays(oracle, b, cw, mm)[1].max() == 0 or fields(lab)["h"] or fields(lab)["defect"]
    assert seen[0] == seen[1] == set(range(mm)), seen
    assert plain == set(range(mm))                                       # ... already without a defect
    assert sum(len(c) for c in craft.family_c(cw, mm).values()) <= 600


def model_parse(b, cw, mm, start, stop, skip=0, toks=None):
    """nearest 3-byte match within cw, extended to mm, greedy -- positions [start + skip, stop) of block b; -> the exit skip"""
    isize = len(b) - 1
    di = start + skip
    while di < stop:
        q = -1
        if di >= 1 and di < isize - 3:
            q = b.rfind(b[di:di + 3], max(0, di - cw), di + 2)           # the largest q <= di - 1: the smallest distance
        if q < 0:
            if toks is not None:
                toks.append((di, 0, b[di]))
            di += 1
            continue
        dist, m = di - q, 3
        for k in range(4, mm + 1):
            if di < isize - k and b[di - dist + k - 1] == b[di + k - 1]:
                m = k
            else:
                break
        if toks is not None:
            toks.append((di, m, dist))
        di += m
    return di - stop


def last32(b, cw, mm, S, skips=range(10)):
    """the transfer function of the 32 positions in front of seam S: entry skip -> exit skip (what k_stream_tails derives)"""
    return [model_parse(b, cw, mm, S - 32, S, s) for s in skips]


@pytest.mark.parametrize("cw,mm", MODEL_WINDOWS)
def test_last32_functions_constant_and_not_in_both_orders(oracle, cw, mm):
    cases = craft.family_c(cw, mm)[N0]
    for i, (lab, b) in enumerate(cases):                                 # the model against the oracle on whole blocks first
        if fields(lab)["defect"] and i % 5:
            continue
        toks = []
        model_parse(b, cw, mm, 0, len(b), 0, toks)
        assert toks == oracle.tokens(b, cw, mm), lab
    kinds = set()
    for lab, b in cases:
        pair = []
        for S in SEAMS:
            f = last32(b, cw, mm, S)
            const = len(set(f)) == 1                                     # constant over all ten nibbles: what the kernel takes as known
            varies = len(set(f[:mm])) > 1                                # not constant over the skips that can occur
            assert const or varies or mm == 5, (lab, f)
            pair.append("c" if const else "n" if varies else "-")
            if varies and not fields(lab)["defect"] and fields(lab)["per"] <= cw:
                assert sorted(f[:mm]) == list(range(mm)), (lab, f)      # back-to-back maximal matches: a permutation of the skip
        kinds.add("".join(pair))
    assert {"cn", "nc", "cc", "nn"} <= kinds, kinds


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_block_ends_cover_every_stream_length_modulo_four(oracle, cw, mm):
    mods, at_end = set(), 0
    fam = craft.family_d(cw, mm)
    assert sorted(fam) == craft.sizes_d() and len(craft.sizes_d()) == 42
    for n, cases in fam.items():
        assert len(cases) == 3
        for lab, b in cases:
            per = fields(lab)["per"]
            ext = b + craft.tail_d(b, per, 48)
            assert len(b) == n and ext[per:] == ext[:-per]
            rc, z = craft.expect(oracle, b, cw, mm)
            assert rc == 0
            mods.add(len(z) % 4)
            pos, ln, _ = craft.token_arrays(oracle, b, cw, mm)
            m = np.nonzero(ln)[0][-1]
            at_end += int(pos[m] + ln[m] >= n - 4)                       # a match up to where the end of the block forbids one
    assert mods == {0, 1, 2, 3}
    assert at_end == 3 * 42
    for per in craft.bodies_d(cw):                                       # laid out in order, each block is followed by its continuation
        blocks, flat = craft.d_flat(cw, mm, per)
        assert flat[per:] == flat[:-per]


# ------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("cw,mm", craft.CHAIN_WINDOWS)
def test_chains_reach_the_chunk_seams_with_a_phase(oracle, cw, mm):
    for tiles in craft.TILES_E:
        for v in range(len(craft.VARIANTS_E)):
            lab, b = craft.chain_e(tiles, v)
            assert len(b) == tiles * TILE + 5
            pos, ln, _ = craft.token_arrays(oracle, b, cw, mm)
            seams = [t * TILE for t in (256, 512) if t * TILE < len(b)]
            if seams:                                                    # a phase at every chunk seam
                assert (craft.entry_skips(pos, ln, seams) != 0).all(), (lab, craft.entry_skips(pos, ln, seams))
            all_seams = np.arange(1, tiles + 1) * TILE
            assert len(set(craft.entry_skips(pos, ln, all_seams).tolist())) == mm       # every phase somewhere in the chain


def test_the_two_chunk_level_chain(oracle):
    cw, mm = 32, 10
    tiles = craft.BIG_TILES_E
    assert (tiles + 1 + 255) // 256 > 64                                 # more than 64 chunks: two chunks per lane in the top scans
    hit = 0
    for v in range(len(craft.VARIANTS_E)):
        lab, b = craft.chain_e(tiles, v)
        assert len(b) == tiles * TILE + 5 > 32 << 20
        pos, ln, _ = craft.token_arrays(oracle, b, cw, mm)
        sk = craft.entry_skips(pos, ln, np.arange(1, tiles + 1) * TILE)
        assert (sk[256 - 1::256] != 0).sum() * 4 >= 3 * 64, lab        # a phase over (at least three in four of) the chunk seams
        hit += int(sk[16384 - 1] != 0 and sk[16385 - 1] != 0)
        if v == 0:
            varies = sum(len(set(last32(b, cw, mm, t * TILE))) > 1 for t in range(1, tiles + 1))
            assert 100 * varies > tiles and varies < tiles, (varies, tiles)
    assert hit >= 1
