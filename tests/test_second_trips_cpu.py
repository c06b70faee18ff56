"""CPU: the thresholds tests/second_trips.py derives from the sources, and every file and batch tests/test_gpu_second_trips.py runs,
held against their references alone -- gzip_members_ref.candidates / index_rule, bgzf_ref.walk, zlib and gzip: the fixtures are what
they claim to be (the candidates lie in the windows named, the clean windows guess right, the failing members fail for the stated
reason only)."""
import gzip
import zlib

import numpy as np
import pytest

import bgzf_ref
import gunzip_ref as G
import gzip_members_ref as R
import second_trips as S


# ---- the thresholds
def test_the_caps_read_from_the_sources():
    assert (S.CRC_TILE, S.CRC_GRID_MAX, S.CRC_FIN_THREADS) == (32768, 1024, 1024)
    assert (S.GZM_WIN, S.SEAM_THREADS) == (32768, 512)
    assert (S.BGZF_WIN, S.BGZF_SEAM_LANES, S.BGZF_EMIT_THREADS) == (65536, 64, 256)
    assert S.JT == 256
    assert S.LOWEST_THREADS == {"bgzf": 256, "gzip members": 256, "unjoin": 256, "unjoin gzip": 1024}
    assert (S.JOIN_FIN_THREADS, S.JOIN_LIFT_GRID, S.JOIN_LIFT_THREADS) == (256, 1024, 256)
    assert (S.GUNZIP_HEADS_GRID, S.GZM_HEADS_GRID) == (65536, 65536)


def test_a_pattern_that_matches_nothing_fails_loudly():
    with pytest.raises(AssertionError):
        S.source_const("hdlz_crc32.h", r"constexpr uint32_t CRC_NO_SUCH_CAP = (\d+)u")
    with pytest.raises(AssertionError):
        S.source_const("hdlz_crc32.h", r"constexpr uint32_t CRC_\w+ = (\d+)u")          # several constants, several values


def test_the_derived_thresholds():
    """whoever changes a cap has to move these figures, and with them the shapes"""
    T = S.THRESHOLDS
    assert T["crc_tiles"] == {"second": 1025, "third": 2049, "ragged": (1025, 2047)}
    # the finishing workgroup numbers ntiles + 1 words: thread 0's second Horner step comes at 1024 TILES (the word is the initial
    # register), a second step over a tile word at 1025
    assert T["crc_finish"] == {"second": 1024, "third": 2048, "ragged": (1024, 2046)}
    assert S.CRC_TILE_COUNTS == [1023, 1024, 1025, 2047, 2048, 2049]
    assert T["gzm_seam"] == {"second": 513, "third": 1025, "fourth": 1537}
    assert T["bgzf_seam"]["second"] == 65 and T["bgzf_seam"]["third"] == 129 and T["bgzf_emit"]["second"] == 257
    assert T["lowest_word"]["bgzf"]["second"] == T["lowest_word"]["gzip members"]["second"] == T["lowest_word"]["unjoin"]["second"] == 65537
    assert T["lowest_word"]["unjoin gzip"]["second"] == 262145                     # 1024 threads there, not 256
    assert T["join_finish"]["second"] == 65537 and T["join_finish"]["third"] == 131073
    assert T["join_gzip_lift"]["second"] == 262145
    assert T["gunzip_heads"]["second"] == T["gzm_heads"]["second"] == 65537
    assert S.MANY == 65536 + 300 and (S.PLANT_HIGH, S.PLANT_LOW) == (256 * 256 + 5, 3 * 256 + 5)
    assert S.JOIN_ROWS == (256 * 256 + 1, 1024 * 256 + 257)
    assert S.join_failed_row(S.JOIN_ROWS[1]) // S.JT == 300 and S.join_failed_row(S.JOIN_ROWS[0]) // S.JT == 256
    assert S.CRC_CALLER_BYTES == 1025 * 32768 + 7
    # the walk of crc_finish, restated: thread i starts at its farthest word and steps down by 1024
    for ntiles, steps0 in ((1023, 1), (1024, 2), (1025, 2), (2047, 2), (2048, 3)):
        j = 0 + ((ntiles - 0) >> 10 << 10)
        assert j // 1024 + 1 == steps0
    assert {S.gzm_shapes()[k] for k in S.gzm_shapes()} == {513 * 32768, 1025 * 32768 + 100, 1537 * 32768}


# ---- the gzip members index
@pytest.mark.parametrize("label", list(S.gzm_shapes()))
def test_gzm_files_hold_exactly_the_planted_candidates(label):
    z, plan = S.gzm_file(label)
    n, win = len(z), S.GZM_WIN
    W = -(-n // win)
    K = -(-W // S.SEAM_THREADS)
    assert K == {"K=2": 2, "K=3 ragged": 3, "K=4": 4}[label]
    assert (-(-W // K) < S.SEAM_THREADS), "the last threads own no window"
    cands = R.candidates(z)
    assert cands == S.gzm_planted(plan)
    owner = lambda p: (p // win) // K                         # noqa: E731  (the seam thread that owns the position's window)
    a, b = plan["two consecutive windows of one thread"]
    assert owner(a) == owner(b) and b // win == a // win + 1
    a, b = plan["the last window of a thread and the first of the next"]
    assert owner(b) == owner(a) + 1 and b // win == a // win + 1
    lo, hi = plan["in front of three empty shares"][0], plan["behind three empty shares"][0]
    assert owner(hi) - owner(lo) == 4 and cands[cands.index(lo) + 1] == hi, "three whole shares without a candidate"
    for i, p in enumerate(plan["seams inside a share"]):
        assert p % win == (i - 3) % win and owner(p - (i - 3) - 1) == owner(p - (i - 3))
    for i, p in enumerate(plan["seams between two shares"]):
        assert p % win == (i - 3) % win and owner(p - (i - 3) - 1) + 1 == owner(p - (i - 3))
    dense = plan["a dense second window"]
    assert len(dense) == 8192 and len({p // win for p in dense}) == 1 and (dense[0] // win) % K == 1
    assert max(cands) // win == W - 1 or label != "K=3 ragged"
    off, out_off = S.index_rule_arrays(z, cands)
    want = R.index_rule(z)
    assert off.tolist() == want[0] and out_off.tolist() == want[1], "the vectorised rule is the rule"
    assert len(set(np.diff(out_off).tolist())) > 50, "the guesses differ: a base that is off shows"
    named = [p for name, ps in plan.items() if name not in ("a dense second window", "every seventh window") for p in ps]
    for p in named:                                           # the guess of the member that ENDS there tells where it began
        b = cands.index(p) - 1
        assert out_off[b + 1] - out_off[b] == 1032 * (off[b + 1] - off[b]) + 258, (p, "a clamped guess: it depends on the candidate in front")
    assert sum(1 for g, sp in zip(np.diff(out_off), np.diff(off)) if 0 < g < 1032 * sp + 258) > 20, "and some guesses are ISIZE words"
    M = len(cands)
    caps = S.gzm_caps(plan, cands)
    assert caps[:2] == [M, M - 1] and caps[4] == 0
    assert cands[caps[2]] // win == dense[0] // win and cands[caps[3]] == plan["two consecutive windows of one thread"][0]


# ---- the BGZF index
@pytest.mark.parametrize("label", list(S.bgzf_shapes()))
def test_bgzf_files_guess_wrong_in_the_windows_named_only(label):
    f, data, fakes = S.bgzf_file(label)
    nwin = S.bgzf_shapes()[label][0]
    w = bgzf_ref.walk(f)
    assert w.status == bgzf_ref.OK and w.eof_marker == 1 and w.file_used == len(f) and -(-len(f) // S.BGZF_WIN) == nwin
    assert gzip.decompress(f) == data
    assert S.bgzf_wrong_guesses(f, w.off[:-1]) == sorted(fakes), "every other window's first header-shaped bytes start a member"
    hits = S.header_shaped(f)
    for win, lands in fakes.items():
        lo = win * S.BGZF_WIN
        first = int(hits[np.searchsorted(hits, lo)])
        assert first == lo + S.FAKE_AT and lo + S.TRUE_AT in w.off and not [o for o in w.off if lo <= o < lo + S.TRUE_AT]
        size = int.from_bytes(f[first + 16:first + 18], "little") + 1
        assert (first + size == lo + S.TRUE_AT) == lands and (lands or not bgzf_ref.is_header(f[first + size:first + size + 18]))
    levels = {(f[o + 18] >> 1) & 3 for o in w.off[:-1]}
    assert levels == {0, 1, 2}, "stored, fixed and dynamic blocks"


def test_bgzf_damage_stops_the_walk_in_windows_70_and_200():
    f, data, _ = S.bgzf_file("259 windows")
    w = bgzf_ref.walk(f)
    for window, first in ((70, False), (200, True)):
        g = S.bgzf_damaged(f, w.off, window, first)
        d = bgzf_ref.walk(g)
        assert d.status == bgzf_ref.E_BAD_HEADER and d.file_used // S.BGZF_WIN == window and d.eof_marker == 0
        assert 0 < d.nmembers < w.nmembers and d.off == w.off[:d.nmembers + 1]
        starts = [o for o in w.off[:-1] if o // S.BGZF_WIN == window]
        assert d.file_used == starts[0 if first else 1]
    in_256 = [b for b, o in enumerate(w.off[:-1]) if o // S.BGZF_WIN >= 256]
    assert len(in_256) >= 6, "a member_cap can end inside window 256 and above"


# ---- more than 65536 streams and members
def test_many_gzip_streams_fail_behind_65536_only(oracle):
    zs, bad = S.many_gzip_streams()
    assert len(zs) == S.MANY and min(bad) >= 65536 and max(bad) == S.MANY - 1
    memo = {z: G.expect(oracle, z, 64) for z in set(zs)}
    assert len(memo) <= 16
    not_ok = {b for b, z in enumerate(zs) if memo[z]["status"] != G.OK}
    assert not_ok == set(bad)
    want = {"wrong magic": G.E_BAD_HEADER, "wrong CRC": G.E_BAD_CHECKSUM, "ISIZE + 1": G.E_BAD_CHECKSUM, "cut trailer": G.E_NO_EOF,
            "reserved flag": G.E_BAD_HEADER}
    for b, why in bad.items():
        assert memo[zs[b]]["status"] == want[why], why
    for z, e in memo.items():
        acc = G.zaccepts(z)
        assert (e["status"] == G.OK) == (acc is not None and acc[1] == len(z)), "stock zlib agrees"
    assert sum(1 for z in zs if z != S.EMPTY_GZ) > 60 and memo[S.EMPTY_GZ]["in_used"] == 20


@pytest.mark.parametrize("planted", [(S.PLANT_HIGH,), (S.PLANT_LOW, S.PLANT_HIGH), ()])
def test_many_gzip_members_fail_where_planted_only(oracle, planted):
    z, off, out_off, datas = S.many_gzip_members(planted)
    assert len(off) == S.MANY + 1 and off[-1] == len(z)
    v = S.verdicts_memoised(oracle, z, off, out_off)
    assert [b for b, (st, _) in enumerate(v) if st != R.OK] == sorted(planted)
    assert all(v[b][0] == R.E_BAD_CHECKSUM for b in planted)
    assert all(d == want for (st, d), want in zip(v, datas) if st == R.OK)
    if not planted:
        assert gzip.decompress(z) == b"".join(datas)
    assert all(S.PLANT_HIGH // S.JT == 256 and S.PLANT_LOW // S.JT == 3 for _ in (0,))


def test_many_bgzf_members():
    f, datas = S.many_bgzf_members()
    w = bgzf_ref.walk(f)
    assert w.status == bgzf_ref.OK and w.nmembers == S.MANY and gzip.decompress(f) == b"".join(datas)
    assert w.out_off == [0] + np.cumsum([len(d) for d in datas]).tolist()
    for b in (S.PLANT_HIGH, S.PLANT_LOW):
        assert datas[b] and f[w.off[b + 1] - 8:w.off[b + 1] - 4] == zlib.crc32(datas[b]).to_bytes(4, "little")
        g = bgzf_ref.with_crc_flipped(f, w.off, [b])
        with pytest.raises(gzip.BadGzipFile):
            gzip.decompress(g)


# ---- the joins
@pytest.mark.parametrize("B", [S.MANY] + list(S.JOIN_ROWS))
def test_pooled_batches_are_ragged_and_their_members_decode(B):
    import joined_ref
    four = B == S.MANY
    blocks, mlen, data = S.pooled_batch(B, four)
    assert len(blocks) == B == len(mlen) and len(data) == sum(map(len, blocks))
    lens = {len(b) for b in blocks}
    assert min(lens) >= 5 and max(lens) <= 64 and len(lens) > 10 and (not four or all(n % 4 == 0 for n in lens))
    pool = S.block_pool(four)
    for p in pool[:20]:
        z, E, pad, m = joined_ref.member_of(p, 32, 10)
        d = zlib.decompressobj(-15)
        assert d.decompress(m + b"\x03\x00") == p and d.eof
    assert int(mlen.sum()) == sum(len(joined_ref.member_of(b, 32, 10)[3]) for b in blocks[:2000]) + int(mlen[2000:].sum())


def test_stored_deflate_is_the_quadratic_builder_and_zlib_reads_it():
    for n in (0, 1, 65535, 65536, 200001):
        d = R.clean_bytes(n, n)
        assert G.header() + S.stored_deflate(d) + G.trailer(d) == R.stored(d) and gzip.decompress(R.stored(d)) == d


def test_literal_data_has_no_match_and_only_short_literals():
    d = S.literal_data(70000)
    assert max(d) < 144
    a = np.frombuffer(d, np.uint8).astype(np.int64)
    tri = a[:-2] * 65536 + a[1:-1] * 256 + a[2:]
    for dist in range(1, 33):
        assert not (tri[dist:] == tri[:-dist]).any()
