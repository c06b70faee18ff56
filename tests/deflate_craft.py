"""Hand-crafted dynamic (BTYPE = 2) deflate blocks, bit by bit (a helper module like checked_ref.py, not a conftest).

Stock zlib's encoder covers a small corner of the headers a decoder must accept -- no 15-bit codes on small inputs, no 7-bit
code-length code, no one-code distance set at symbol 29, never 258 as symbol 284 + 31 extra -- and none of those it must reject.
This module writes such blocks in pure Python: `emit_block` takes the code lengths, the tokens and, if wanted, the exact sequence of
code-length-code operations; `catalogue()` is a list of named cases with their expectation (the plain bytes, computed here from the
tokens, or the status of the rejection); `random_stream()` draws whole streams; `header_flips()` damages a stream inside a block header.
Nothing here looks at a decoder: tests/test_crafted_trees_cpu.py holds all of it against stock zlib and the C oracle.
The second half does for block BODIES what the first does for headers: `geometry_stream`, `geometry_mixed` and `geometry_rejected` put
match distances and lengths on the ring thresholds of the inflate kernels, in fixed blocks (`emit_fixed_block`) and in dynamic ones whose
code comes from the token frequencies (`frequency_lengths`); tests/test_match_geometry_cpu.py holds those against zlib and the oracle.
The third part, `chain_cases`, puts whole streams on the limits of the two whole-GPU inflate chains -- list sizes, bit budgets, piece
boundaries, false block headers written into the stream by literals -- with the verdict each must get; tests/test_chain_cases_cpu.py
measures them, tests/test_gpu_chain_verdicts.py asserts the verdicts."""
import functools
import random
import zlib

OK, E_BAD_DISTANCE, E_BAD_SYMBOL, E_BAD_TREE = 0, 4, 7, 10
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)       # RFC1951 3.2.7
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DEXTRA = tuple(0 if c < 2 else c // 2 - 1 for c in range(30))
DBASE = tuple(1 + sum(1 << DEXTRA[k] for k in range(c)) for c in range(30))
assert DBASE[29] + (1 << DEXTRA[29]) - 1 == 32768 and LBASE[27] + 31 == 258


class Bits(object):
    """LSB-first bit writer; Huffman codes go in MSB first (RFC1951 3.1.1)"""

    def __init__(self):
        self.out, self.acc, self.n, self.pos = bytearray(), 0, 0, 0

    def put(self, v, nb):
        self.acc |= (v & ((1 << nb) - 1)) << self.n
        self.n += nb
        self.pos += nb
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, cl):
        self.put(cl[0], cl[1])                         # (canonical() hands the codes out bit-reversed)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def kraft(lengths, unit=15):
    """the code space the lengths take, in units of 2^-unit: 2^unit = complete"""
    return sum(1 << (unit - l) for l in lengths if l)


def canonical(lengths):
    """symbol -> (code with its bits reversed: as Bits.put takes it, length), RFC1951 3.2.2; for a set that is no prefix code the same
    arithmetic, truncated to the length"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (int(format(nxt[l] & ((1 << l) - 1), "0%db" % l)[::-1], 2), l)
            nxt[l] += 1
    return out


def complete_code(n, rng, max_len, shuffle=True):
    """n code lengths with Kraft sum exactly 1 whose longest is exactly max_len where n allows it (n > max_len; for more than 2^max_len
    codes the longest is as short as n allows): the chain 1, 2, .., max_len, max_len with random leaves shorter than max_len split"""
    if n == 1:
        return [1]                                     # (the one incomplete set a decoder accepts)
    max_len = min(max_len, n - 1)
    while (1 << max_len) < n:
        max_len += 1
    cnt = [0] * (max_len + 2)
    for l in range(1, max_len + 1):
        cnt[l] = 1
    cnt[max_len] = 2
    for _ in range(n - (max_len + 1)):
        open_ = [l for l in range(1, max_len) if cnt[l]]
        l = rng.choices(open_, [cnt[l] for l in open_])[0]
        cnt[l] -= 1
        cnt[l + 1] += 2
    lens = [l for l in range(1, max_len + 1) for _ in range(cnt[l])]
    assert len(lens) == n and kraft(lens) == 1 << 15 and max(lens) == max_len
    if shuffle:
        rng.shuffle(lens)
    return lens


def rle_ops(lengths):
    """the run-length form of a length list: 0..15 as ints, repeats as (16 | 17 | 18, value of the extra field)"""
    ops, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                ops.append((18, k - 11))
                run -= k
            if run >= 3:
                ops.append((17, run - 3))
                run = 0
            ops += [0] * run
        else:
            ops.append(v)
            run -= 1
            while run >= 3:
                k = min(run, 6)
                ops.append((16, k - 3))
                run -= k
            ops += [v] * run
        i = j
    return ops


def op_sym(op):
    return op[0] if isinstance(op, tuple) else op


def op_rep(op):
    return 1 if not isinstance(op, tuple) else op[1] + (11 if op[0] == 18 else 3)


def balanced(n):
    """n lengths of a complete code, as even as possible (shortest first)"""
    if n == 1:
        return [1]
    k = n.bit_length() - 1
    if 1 << k == n:
        return [k] * n
    return [k] * ((2 << k) - n) + [k + 1] * (2 * (n - (1 << k)))


def default_cl_lens(ops):
    """19 lengths of a complete code-length code over the symbols the operations use (the more frequent, the shorter)"""
    freq = {}
    for op in ops:
        freq[op_sym(op)] = freq.get(op_sym(op), 0) + 1
    if len(freq) == 1:                                 # a code-length code of one code is incomplete: a second, unused one
        freq[0 if 0 not in freq else 1] = 0
    syms = sorted(freq, key=lambda s: (-freq[s], s))
    cl = [0] * 19
    for s, l in zip(syms, balanced(len(syms))):
        cl[s] = l
    return cl


def length_symbol(length):
    s = max(k for k in range(29) if LBASE[k] <= length)
    return 257 + (28 if length == 258 else s)


def distance_symbol(dist):
    return max(k for k in range(30) if DBASE[k] <= dist)


def emit_block(w, ll, dl, tokens, final, ops=None, cl_lens=None, hclen=None, rle=True, eob=True):
    """one dynamic block into the Bits `w`.  ll: HLIT + 257 literal/length code lengths, dl: HDIST + 1 distance code lengths (the counts
    written are the lists' lengths, whatever they are); tokens: ints (literals) and (length, distance[, length symbol]);
    ops: the code-length-code operations (default: rle_ops or one per length); cl_lens: the 19 code-length-code lengths by symbol
    (default: a complete code over the used symbols); hclen: how many of them are written (default: as few as a header may).
    -> dict: span = (first bit, end bit) of the header, and what the coverage assertions ask about"""
    lengths = list(ll) + list(dl)
    if ops is None:
        ops = rle_ops(lengths) if rle else list(lengths)
    if cl_lens is None:
        cl_lens = default_cl_lens(ops)
    assert len(cl_lens) == 19 and max(cl_lens) <= 7
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if cl_lens[ORDER[i]]])
    assert 4 <= hclen <= 19 and all(cl_lens[ORDER[i]] == 0 for i in range(hclen, 19))
    start = w.pos
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(len(ll) - 257, 5)
    w.put(len(dl) - 1, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_lens[ORDER[i]], 3)
    cc = canonical(cl_lens)
    idx, cross = 0, False
    for op in ops:
        w.code(cc[op_sym(op)])
        if isinstance(op, tuple):
            w.put(op[1], {16: 2, 17: 3, 18: 7}[op[0]])
            cross = cross or idx < len(ll) < idx + op_rep(op)
        idx += op_rep(op)
    end = w.pos
    lc, dc = canonical(ll), canonical(dl)
    for t in tokens:
        if isinstance(t, int):
            w.code(lc[t])
            continue
        length, dist = t[0], t[1]
        ls = t[2] if len(t) > 2 else length_symbol(length)
        w.code(lc[ls])
        assert 0 <= length - LBASE[ls - 257] < (1 << LEXTRA[ls - 257]) or length == LBASE[ls - 257]
        w.put(length - LBASE[ls - 257], LEXTRA[ls - 257])
        ds = distance_symbol(dist)
        w.code(dc[ds])
        w.put(dist - DBASE[ds], DEXTRA[ds])
    if eob and 256 in lc:
        w.code(lc[256])
    return dict(span=(start, end), offset=start & 7, ncoded=sum(1 for l in ll if l), ndcoded=sum(1 for l in dl if l),
                max_ll=max(ll), max_dl=max(dl), max_cl=max(cl_lens), cross=cross, hclen=hclen,
                rle=any(isinstance(op, tuple) for op in ops))


def emit_fixed_prefix(w, m):
    """a fixed-Huffman block (not final) of m nine-bit literals: 10 + 9 m bits, so the next header starts at bit (2 + m) mod 8 behind
    a byte-aligned start -> the literals"""
    w.put(0, 1)
    w.put(1, 2)
    lits = [144 + (7 * k) % 112 for k in range(m)]
    for v in lits:
        w.put(int(format(0b110010000 + (v - 144), "09b")[::-1], 2), 9)
    w.put(0, 7)
    return bytes(lits)


PREFIX_FOR_OFFSET = {(2 + m) % 8: m for m in range(8)}           # m literals in front -> bit offset of the next header


def apply_tokens(out, tokens):
    """the plain bytes of the tokens appended to the bytearray `out` (None when a distance reaches before the start)"""
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        length, dist = t[0], t[1]
        if dist > len(out):
            return None
        if dist >= length:
            out += out[len(out) - dist:len(out) - dist + length]
        else:
            pat = bytes(out[len(out) - dist:])
            out += (pat * (length // dist + 1))[:length]
    return out


def wrap(body, plain):
    return b"\x78\x9c" + body + zlib.adler32(plain).to_bytes(4, "big")


class Case(object):
    """name; z: the zlib-framed stream; raw: the deflate stream alone; plain (None for a rejected one) and status; blocks: emit_block's
    records, their spans in bits of z"""

    def __init__(self, name, w, plain, status, blocks):
        self.name, self.raw, self.status = name, w.bytes(), status
        self.plain = bytes(plain) if status == OK else None
        self.z = wrap(self.raw, self.plain or b"")
        self.blocks = blocks
        self.spans = [(b["span"][0] + 16, b["span"][1] + 16) for b in blocks]

    def __repr__(self):
        return "Case(%s)" % self.name


def one_block(name, ll, dl, tokens, status=OK, prefix_offset=None, **kw):
    """a stream of one final crafted block, behind a fixed block that puts its header at the given bit offset if one is asked for"""
    w, out = Bits(), bytearray()
    if prefix_offset is not None:
        out += emit_fixed_prefix(w, PREFIX_FOR_OFFSET[prefix_offset])
        assert w.pos & 7 == prefix_offset
    b = emit_block(w, ll, dl, tokens, True, **kw)
    plain = apply_tokens(out, tokens) if status == OK else None
    assert status != OK or plain is not None
    return Case(name, w, plain, status, [b])


def sparse(n, lens):
    """n lengths, zero but for the dict"""
    out = [0] * n
    for s, l in lens.items():
        out[s] = l
    return out


def all_symbols_tokens():
    """every literal, > 32 KiB of them; every length symbol and every distance symbol at its lowest and highest extra value; 258 as
    symbol 285 and as 284 + 31"""
    toks = [(k * 167 + (k >> 8)) & 255 for k in range(32768 + 256)]
    assert set(toks) == set(range(256))
    lens = []
    for s in range(29):
        lens += [(LBASE[s], 257 + s), (LBASE[s] + (1 << LEXTRA[s]) - 1, 257 + s)]
    assert (258, 284) in lens and (258, 285) in lens
    dists = []
    for c in range(30):
        dists += [DBASE[c], DBASE[c] + (1 << DEXTRA[c]) - 1]
    for k in range(max(len(lens), len(dists))):
        ln, ls = lens[k % len(lens)]
        toks.append((ln, dists[(k * 7) % len(dists)], ls))
        toks.append((k * 31) & 255)
        ln, ls = lens[(k * 11) % len(lens)]
        toks.append((ln, dists[k % len(dists)], ls))
    return toks


def tokens_for(rng, ll, dl, n, produced):
    """n random tokens that only use coded symbols and distances that reach no further back than `produced` bytes + their own output"""
    lits = [s for s in range(256) if s < len(ll) and ll[s]]
    lsyms = [s for s in range(257, min(len(ll), 286)) if ll[s]]
    dsyms = [c for c in range(min(len(dl), 30)) if dl[c]]
    toks = []
    for _ in range(n):
        reach = [c for c in dsyms if DBASE[c] <= produced]
        if lsyms and reach and (not lits or rng.random() < 0.18):
            ls, c = rng.choice(lsyms), rng.choice(reach)
            length = LBASE[ls - 257] + rng.choice((0, (1 << LEXTRA[ls - 257]) - 1, rng.randrange(1 << LEXTRA[ls - 257])))
            dist = min(produced, DBASE[c] + rng.choice((0, (1 << DEXTRA[c]) - 1, rng.randrange(1 << DEXTRA[c]))))
            toks.append((length, dist, ls))
            produced += length
        elif lits:
            toks.append(rng.choice(lits))
            produced += 1
        else:
            break
    return toks


def random_block_lengths(rng, count=None, max_len=None, dist_kind=None):
    """(ll, dl) of one random block: HLIT and HDIST, `count` coded literal/length symbols among them (256 always), a complete code"""
    if count is None:
        count = rng.choice((2, 10, 143, 144, 145, 285, 286, rng.randint(2, 286), rng.randint(2, 60)))
    if max_len is None:
        max_len = rng.choice((7, 9, 12, 15))
    coded = [256] + rng.sample([s for s in range(286) if s != 256], count - 1)
    nlen = rng.randint(max(257, max(coded) + 1), 286)
    ll = [0] * nlen
    for s, l in zip(coded, complete_code(count, rng, max_len)):
        ll[s] = l
    kind = dist_kind or rng.choice(("none", "one", "several", "several"))
    if kind == "none":
        dl = [0] * rng.randint(1, 30)
    elif kind == "one":
        c = rng.randrange(30)
        dl = sparse(rng.randint(c + 1, 30), {c: 1})
    else:
        k = rng.randint(2, 30)
        dsy = rng.sample(range(30), k)
        dl = [0] * rng.randint(max(dsy) + 1, 30)
        for c, l in zip(dsy, complete_code(k, rng, rng.choice((5, 7, 9, 12, 15)))):
            dl[c] = l
    return ll, dl


SPOILS = ("hlit_288", "hdist_32", "single_distance_code_of_length_5")


def random_stream(seed, nblocks, tokens_per_block, spoil=None):
    """-> Case: nblocks random crafted blocks (see random_block_lengths, tokens_for), half of the streams behind a fixed block that
    moves the first header off the byte boundary.  spoil = (k, one of SPOILS): block k's header is one a decoder must reject although
    everything in the block can be decoded -- the counts raised over 286 / 30 with zero lengths, or a distance set (unused: the block
    has literals only) of one 5-bit code; the blocks in front of it are those of the unspoiled stream"""
    rng = random.Random(seed)
    w, out, blocks = Bits(), bytearray(), []
    if rng.random() < 0.5:
        out += emit_fixed_prefix(w, rng.randrange(8))
    for k in range(nblocks):
        ll, dl = random_block_lengths(rng)
        if spoil and spoil[0] == k and spoil[1] == "single_distance_code_of_length_5":
            dl = [0] * len(dl)
        toks = tokens_for(rng, ll, dl, tokens_per_block, len(out))
        if spoil and spoil[0] == k:
            if spoil[1] == "hlit_288":
                ll = ll + [0] * (288 - len(ll))
            elif spoil[1] == "hdist_32":
                dl = dl + [0] * (32 - len(dl))
            else:
                dl[len(dl) // 2] = 5
        kw = {}
        if rng.random() < 0.15:                        # a code-length code of all 19 symbols, up to 7 bits
            kw["cl_lens"] = complete_code(19, rng, 7)
        blocks.append(emit_block(w, ll, dl, toks, k == nblocks - 1, rle=rng.random() < 0.6, **kw))
        assert apply_tokens(out, toks) is not None
    if spoil:
        return Case("random_%d %s in block %d" % (seed, spoil[1], spoil[0]), w, None, E_BAD_TREE, blocks)
    return Case("random_%d" % seed, w, out, OK, blocks)


def _alternating(offset, rng):
    """six blocks, a 286-symbol 15-bit tree and a two-symbol tree in turn, the first header at bit `offset` of its byte"""
    w, out, blocks = Bits(), bytearray(), []
    if offset:
        out += emit_fixed_prefix(w, PREFIX_FOR_OFFSET[offset])
    assert w.pos & 7 == offset
    for k in range(6):
        if k % 2 == 0:
            ll, dl = complete_code(286, rng, 15), complete_code(30, rng, 15)
        else:
            ll, dl = sparse(257, {97 + k: 1, 256: 1}), [0]
        toks = tokens_for(rng, ll, dl, 40, len(out))
        blocks.append(emit_block(w, ll, dl, toks, k == 5, rle=k != 2))
        apply_tokens(out, toks)
    assert blocks[0]["offset"] == offset
    return Case("alternating_offset%d" % offset, w, out, OK, blocks)


def catalogue():
    """-> [Case]: the named headers, valid (status OK, .plain) and rejected (.status)"""
    rng = random.Random(20261019)
    cs = []
    # ---- valid
    ll, dl = sorted(complete_code(286, rng, 15)), sorted(complete_code(30, rng, 15))
    ll, dl = ll[100:] + ll[:100], dl[7:] + dl[:7]          # (runs of equal lengths, so that the run-length form has something to do)
    toks = all_symbols_tokens()
    cs.append(one_block("all_symbols_rle", ll, dl, toks, rle=True))
    cs.append(one_block("all_symbols_plain", ll, dl, toks, rle=False))
    assert cs[0].blocks[0]["rle"] and not cs[1].blocks[0]["rle"] and cs[0].plain == cs[1].plain and len(cs[0].plain) < 65536 - 16
    cs.append(one_block("eob_only", sparse(257, {256: 1}), [0], []))
    small = sparse(260, {97: 2, 98: 3, 99: 3, 256: 3, 257: 3, 258: 3, 259: 3})
    assert kraft(small) == 1 << 15
    for c in (0, 3, 29):
        lits = [97 + (k * k) % 3 for k in range(DBASE[c] + 5)]
        far = DBASE[c] + (1 << DEXTRA[c]) - 1
        toks = lits + [(3, DBASE[c]), 98, (5, DBASE[c] + 1 if DEXTRA[c] else DBASE[c]), (4, min(far, len(lits) + 9)), 99, (5, DBASE[c])]
        cs.append(one_block("one_distance_code_at_%d" % c, small, sparse(c + 1, {c: 1}), toks))
    b = one_block("repeat16_crosses", sparse(260, {97: 2, 98: 2, 256: 3, 257: 3, 258: 3, 259: 3}), [3] * 8,
                  [97, 98, 97, 97, (3, 2), (4, 1), 98, (5, 7), (5, 5), (3, 16)], prefix_offset=5)
    assert b.blocks[0]["cross"] and (16, 3) in rle_ops(sparse(260, {97: 2, 98: 2, 256: 3, 257: 3, 258: 3, 259: 3}) + [3] * 8)
    cs.append(b)
    b = one_block("repeat18_crosses", sparse(270, {97: 2, 98: 2, 256: 2, 257: 2}), sparse(13, {12: 1}),
                  [97 + (k & 1) * (k % 3 == 0) for k in range(70)] + [(3, 65), 98, (3, 70)], prefix_offset=3)
    assert b.blocks[0]["cross"]
    cs.append(b)
    ll, dl = random_block_lengths(random.Random(7), count=40, max_len=9, dist_kind="several")
    ops = rle_ops(ll + dl)
    freq = {}
    for op in ops:
        freq[op_sym(op)] = freq.get(op_sym(op), 0) + 1
    cl = [0] * 19                                          # all 19 symbols coded, the most frequent with the LONGEST codes
    for s, l in zip(sorted(range(19), key=lambda s: (-freq.get(s, 0), s)), sorted(complete_code(19, rng, 7), reverse=True)):
        cl[s] = l
    b = one_block("code_length_code_7_bits", ll, dl, tokens_for(random.Random(8), ll, dl, 60, 0), ops=ops, cl_lens=cl, hclen=19)
    assert b.blocks[0]["max_cl"] == 7 and min(cl) > 0
    cs.append(b)
    # HCLEN = 5 -- 16, 17, 18, 0, 8 -- is the least that gives any symbol a length: 256 codes of 8 bits
    b = one_block("hclen_smallest", [8] * 255 + [0, 8], [0], [k * 3 & 255 if k * 3 & 255 != 255 else 1 for k in range(50)],
                  cl_lens=sparse(19, {8: 1, 0: 2, 16: 3, 18: 3}), prefix_offset=7)
    assert b.blocks[0]["hclen"] == 5
    cs.append(b)
    flat = [8] * 226 + [9] * 60
    assert kraft(flat) == 1 << 15
    dl = [4, 4] + [5] * 28
    cs.append(one_block("flat_8_9", flat, dl, tokens_for(random.Random(9), flat, dl, 80, 0), prefix_offset=1))
    for n in (143, 144, 145, 286):
        r = random.Random(n)
        ll, dl = random_block_lengths(r, count=n, max_len=15, dist_kind="several")
        b = one_block("coded_%d" % n, ll, dl, tokens_for(r, ll, dl, 120, 0), prefix_offset=(n % 7) + 1)
        assert b.blocks[0]["ncoded"] == n
        cs.append(b)
    for offset in range(8):
        cs.append(_alternating(offset, rng))
    # ---- rejected in the header: HDLZ_E_BAD_TREE
    good, gd = sparse(258, {97: 1, 256: 2, 257: 2}), [1, 1]

    def bad(name, ll=good, dl=gd, status=E_BAD_TREE, toks=(), **kw):
        cs.append(one_block(name, ll, dl, list(toks), status=status, **kw))
    bad("first_op_is_16", ops=[(16, 0)] + (good + gd)[3:], cl_lens=sparse(19, {0: 1, 1: 2, 2: 3, 16: 3}))
    bad("repeat_overruns", ops=(good + gd)[:-2] + [(16, 0)], cl_lens=sparse(19, {0: 1, 1: 2, 2: 3, 16: 3}))
    bad("repeat18_overruns", ops=(good + gd)[:-2] + [(18, 0)], cl_lens=sparse(19, {0: 1, 1: 2, 2: 3, 18: 3}))
    bad("no_end_of_block", ll=sparse(258, {97: 1, 98: 2, 257: 2}))
    bad("literals_oversubscribed", ll=sparse(258, {97: 1, 256: 1, 257: 1}))
    bad("literals_incomplete_two_codes", ll=sparse(258, {97: 2, 256: 2}))
    bad("literals_incomplete_2_2_2_15", ll=sparse(258, {97: 2, 98: 2, 256: 2, 257: 15}))
    bad("distances_oversubscribed", dl=[1, 1, 1])
    bad("distances_incomplete_two_codes", dl=[2, 2])
    bad("distances_30_of_5_bits", dl=[5] * 30)
    bad("single_distance_code_of_length_5", dl=[0, 0, 5])
    bad("single_distance_code_of_length_2_at_0", dl=[2])
    bad("end_of_block_only_length_3", ll=sparse(257, {256: 3}), dl=[0])
    bad("end_of_block_only_length_15", ll=sparse(257, {256: 15}), dl=[0])
    bad("code_length_code_incomplete", cl_lens=sparse(19, {0: 2, 1: 2, 2: 2}), rle=False)
    bad("code_length_code_oversubscribed", cl_lens=sparse(19, {0: 1, 1: 1, 2: 1}), rle=False)
    bad("hlit_287", ll=good + [0] * 29)
    bad("hlit_288", ll=good + [0] * 30)
    bad("hdist_31", dl=gd + [0] * 29)
    bad("hdist_32", dl=gd + [0] * 30)
    # ---- rejected in the block body
    w = Bits()
    b = emit_block(w, small, [1], [97, 98, 99], True, eob=False)
    w.code(canonical(small)[257])
    w.put(1, 1)                                            # the unused code of the one-code distance set
    w.code(canonical(small)[256])
    cs.append(Case("unused_code_of_one_distance_code", w, None, E_BAD_SYMBOL, [b]))
    w = Bits()
    b = emit_block(w, sparse(257, {256: 1}), [0], [], True, eob=False)
    w.put(1, 1)                                            # the unused code of the one-code literal/length set
    w.put(0, 1)
    cs.append(Case("unused_code_of_one_literal_code", w, None, E_BAD_SYMBOL, [b]))
    bad("distance_before_the_start", ll=small, dl=[2, 2, 2, 2], status=E_BAD_DISTANCE, toks=[97, 98, (3, 3)])
    assert len(set(c.name for c in cs)) == len(cs)
    return cs


def truncations(case):
    """the stream cut at every byte length from 5 up to (not including) its own"""
    return [case.z[:n] for n in range(5, len(case.z))]


def header_flips(z, spans, rng, k):
    """k copies of z, each with one bit flipped inside a block header (spans: the headers' bit ranges in z)"""
    out = []
    for _ in range(k):
        a, b = spans[rng.randrange(len(spans))]
        bit = rng.randrange(a, b)
        m = bytearray(z)
        m[bit >> 3] ^= 1 << (bit & 7)
        out.append(bytes(m))
    return out


def random_small(n=300):
    """the n small random streams of the suite: 1 to 4 blocks of 40 tokens"""
    return [random_stream(1000 + s, 1 + s % 4, 40) for s in range(n)]


TRUNCATED = ("repeat18_crosses", "code_length_code_7_bits")     # the small valid streams that are cut at every byte


@functools.lru_cache(None)
def suite():
    """what both test files run, built once per process -> dict: catalogue [Case], random [Case] (300 small streams), cuts [bytes] (the
    TRUNCATED streams at every length: stock zlib gives no verdict on a cut stream, so only the oracle judges them), flips [bytes]
    (three header flips of each of 40 random streams)"""
    cat, rnd = catalogue(), random_small()
    by_name = dict((c.name, c) for c in cat)
    rng = random.Random(40)
    flips = [m for c in rnd[3::7][:40] for m in header_flips(c.z, c.spans, rng, 3)]
    assert len(flips) == 120
    return dict(catalogue=cat, random=rnd, cuts=[z for n in TRUNCATED for z in truncations(by_name[n])], flips=flips)


@functools.lru_cache(None)
def large():
    """the streams of the whole-GPU test -> [(label, stream, plain or None)]: six random streams of 40 blocks x 1500 tokens, the
    all-symbols catalogue stream, eight header flips of each, and three of the random streams with a spoiled header in the middle"""
    valid = [random_stream(7000 + k, 40, 1500) for k in range(6)] + [suite()["catalogue"][0]]
    rng = random.Random(41)
    out = [(c.name, c.z, c.plain) for c in valid]
    for k, kind in enumerate(SPOILS):
        c = random_stream(7000 + k, 40, 1500, spoil=(17 + k, kind))
        out.append((c.name, c.z, None))
    for c in valid:
        out += [("%s flip %d" % (c.name, k), m, None) for k, m in enumerate(header_flips(c.z, c.spans, rng, 8))]
    return out


# ------------------------------------------------------------------------------------------------------------------ match geometry
# Block BODIES: token lists whose distances and lengths sit on the comparisons by which every inflate decoder chooses between its LDS ring,
# its own flushed output and a marker.  tests/test_match_geometry_cpu.py reads the kernels' constants and fails when a grid below no
# longer holds a threshold and its two neighbours.
FIXED_LL = (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 8            # RFC1951 3.2.6
FIXED_DL = (5,) * 30

GEO_DISTANCES = (
    1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14,    # periods below a 16-byte step: a copy that overlaps itself (every `i % D` arm; 3, 4, 5: a dword)
    15, 16, 17,                                       # the 16 source bytes of a step (k_inflate_tok's far load, k_inflate_grp's lanes)
    18, 19, 20,                                       # k_inflate_tok: a round advances the output by at most 19 bytes
    31, 32, 33,                                       # k_inflate_grp: RB - NEAR = 32, two steps
    47, 48, 49,                                       # k_inflate_tok with a 64-byte ring: NEAR = 64 - 16
    63, 64, 65,                                       # CHUNK, DCHUNK: the 64-byte flush line; a wave's lanes
    75, 76, 77,                                       # k_inflate_tok: URGENT = RINGB - 52
    94, 95, 96,                                       # k_inflate_tok: URGENT + 19, the most unflushed bytes when a far load is issued
    108, 109, 110,
    111, 112, 113,                                    # k_inflate_tok: NEAR = RINGB - 16, ring or far load
    114, 115, 116,                                    # k_inflate_tok: NEAR + 3, the dword alignment of the source
    117, 118, 119, 120, 121, 122, 123, 124, 125, 126,
    127, 128, 129,                                    # k_inflate_tok: RINGB
    130, 131,
    255, 256, 257,                                    # the longest match but one byte or two; a quarter of HRING
    447, 448, 449,                                    # k_inflate_dyn: WCAP
    511, 512, 513,                                    # k_inflate_dyn: the 512 of DRING - 512; half of FLUSH
    767, 768, 769,                                    # k_par_emit: SPAN
    895, 896, 897,                                    # k_par_emit, k_any_*: HREACH = HRING - 128, ring or marker
    1023, 1024, 1025,                                 # HRING; k_inflate_grp: FLUSH
    1277, 1278, 1279,                                 # k_inflate_dyn: DRING - 512 - 258
    1280, 1281,                                       # HRING + 256
    1471, 1472, 1473,                                 # k_inflate_dyn: DRING - 512 - 64
    1519, 1520, 1521,                                 # k_inflate_dyn: DRING - 512 - 16
    1532, 1533, 1534,                                 # k_inflate_dyn: DRING - 512 - 3
    1535, 1536, 1537,                                 # k_inflate_dyn: DRING - 512, in the ring or out[src]
    2015, 2016, 2017,                                 # k_inflate_grp: NEAR = RB - 32, ring or HBM
    2031, 2032, 2033,                                 # k_inflate_grp: RB - 16, one step below the ring's size
    2047, 2048, 2049,                                 # RB, DRING
    4095, 4096, 4097,                                 # powers of two up to the window: the distance codes' bases + 1 ...
    8191, 8192, 8193,
    16383, 16384, 16385,
    24576, 24577,                                     # ... the last distance code's base
    32767, 32768)                                     # the window
GEO_LENGTHS = (
    3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14,          # the shortest matches: within one 16-byte step; k_inflate_tok's dwords
    15, 16, 17,                                       # one step of 16 bytes and its neighbours
    18, 19, 20,                                       # k_inflate_tok: the 19 bytes of a round
    31, 32, 33, 34, 35,                               # two steps; k_inflate_grp: RB - NEAR
    63, 64, 65, 66, 67,                               # CHUNK, DCHUNK: a flush line; a wave's lanes
    127, 128, 129, 130, 131,                          # k_inflate_tok: RINGB; k_par_emit: HRING - HREACH
    192, 227,                                         # three flush lines; the base of length symbol 284
    255, 256, 257, 258)                               # 257 = symbol 284 + 30, 258 = symbol 285
assert len(GEO_DISTANCES) == len(set(GEO_DISTANCES)) == 116 and len(GEO_LENGTHS) == len(set(GEO_LENGTHS)) == 39
GEO_KINDS = ("fixed", "dynamic")


def emit_fixed_block(w, tokens, final):
    """one fixed-Huffman block (BTYPE = 1) into the Bits `w` from the token lists emit_block takes: the code of RFC1951 3.2.6 through
    canonical(), 258 as symbol 285 unless the token names its length symbol, 5-bit distance codes, the end-of-block code
    -> dict: span = (first bit, end bit) of the three header bits"""
    start = w.pos
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    emit_tokens(w, FIXED_LL, FIXED_DL, tokens)
    return dict(span=(start, start + 3), offset=start & 7)


def emit_tokens(w, ll, dl, tokens):
    """the tokens and an end-of-block code in the codes of the lengths ll / dl (what emit_block writes behind its header)"""
    lc, dc = canonical(ll), canonical(dl)
    for t in tokens:
        if isinstance(t, int):
            w.code(lc[t])
            continue
        ls = t[2] if len(t) > 2 else length_symbol(t[0])
        w.code(lc[ls])
        assert 0 <= t[0] - LBASE[ls - 257] < (1 << LEXTRA[ls - 257]) or t[0] == LBASE[ls - 257]
        w.put(t[0] - LBASE[ls - 257], LEXTRA[ls - 257])
        ds = distance_symbol(t[1])
        w.code(dc[ds])
        w.put(t[1] - DBASE[ds], DEXTRA[ds])
    w.code(lc[256])


def token_bits(ll, dl, tokens):
    """the number of bits each token takes in the codes of the lengths ll / dl"""
    out = []
    for t in tokens:
        if isinstance(t, int):
            out.append(ll[t])
            continue
        ls, ds = t[2] if len(t) > 2 else length_symbol(t[0]), distance_symbol(t[1])
        out.append(ll[ls] + LEXTRA[ls - 257] + dl[ds] + DEXTRA[ds])
    return out


def limited_lengths(freq, limit=15):
    """symbol -> code length of a Huffman code for the frequencies (a dict), no code longer than `limit`: while the tree is too deep the
    frequencies are halved (rounded up), which ends at the latest with all of them 1, a balanced tree.  One symbol: length 1"""
    import heapq
    syms = sorted(freq)
    if len(syms) == 1:
        return {syms[0]: 1}
    f = dict(freq)
    while True:
        heap = [(f[s], s, (s,)) for s in syms]
        heapq.heapify(heap)
        depth = dict.fromkeys(syms, 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= limit:
            return depth
        f = dict((s, (v + 1) // 2) for s, v in f.items())


def frequency_lengths(tokens):
    """(ll, dl) of a length-limited (15 bits) Huffman code from the frequencies of the tokens' symbols, 256 always coded; a single used
    distance symbol gets length 1, no match at all gives dl = [0].  Frequent matches get short codes this way, so that several of them
    fall into one 64-bit decode window"""
    lf, df = {256: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            lf[t] = lf.get(t, 0) + 1
            continue
        ls, ds = t[2] if len(t) > 2 else length_symbol(t[0]), distance_symbol(t[1])
        lf[ls] = lf.get(ls, 0) + 1
        df[ds] = df.get(ds, 0) + 1
    ll = sparse(max(257, max(lf) + 1), limited_lengths(lf))
    dl = sparse(max(df) + 1, limited_lengths(df)) if df else [0]
    assert len(lf) == 1 or kraft(ll) == 1 << 15
    assert len(df) <= 1 or kraft(dl) == 1 << 15
    return ll, dl


def geometry_case(name, blocks_of_tokens, kind, status=OK, **attrs):
    """-> Case: one block per token list, all fixed or all dynamic with frequency_lengths of their own.  On top of Case's fields: tokens
    (all of them), token_pos (the bit in .raw at which each begins; + 16: in .z), kind and whatever `attrs` name"""
    w, out, blocks, pos, tokens = Bits(), bytearray(), [], [], []
    for k, toks in enumerate(blocks_of_tokens):
        final = k == len(blocks_of_tokens) - 1
        if kind == "fixed":
            ll, dl = FIXED_LL, FIXED_DL
            blocks.append(emit_fixed_block(w, toks, final))
        else:
            assert kind == "dynamic"
            ll, dl = frequency_lengths(toks)
            blocks.append(emit_block(w, ll, dl, toks, final))
        p = blocks[-1]["span"][1]
        for nb in token_bits(ll, dl, toks):
            pos.append(p)
            p += nb
        assert p + ll[256] == w.pos
        tokens += toks
        if out is not None:
            out = apply_tokens(out, toks)
    assert (out is not None) == (status == OK), name
    c = Case(name, w, out, status, blocks)
    c.tokens, c.token_pos, c.kind = tokens, pos, kind
    for k, v in attrs.items():
        setattr(c, k, v)
    return c


def geometry_stream(D, kind, long_preamble=False):
    """-> Case (+ .D, .first_match: the number of literals in front of the first match): one block, seeded by D.  A preamble of
    max(D, 64) + randrange(64) uniformly random literals -- a source that is off by one byte shows, and the first match starts at any
    phase of a 64-byte line; long_preamble: at least 4400 of them, which is above HDLZ_INFLATE_PAR_MIN and ANY_MIN in both codings --,
    then every length of GEO_LENGTHS once, in random order, at distance D, with 0 to 3 random literals behind each (the lane decoder's
    groups of three literals and a match)"""
    rng = random.Random(D)
    npre = max(D, 64, 4400 if long_preamble else 0) + rng.randrange(64)
    toks = [rng.randrange(256) for _ in range(npre)]
    lens = list(GEO_LENGTHS)
    rng.shuffle(lens)
    for l in lens:
        toks.append((l, D))
        toks += [rng.randrange(256) for _ in range(rng.randrange(4))]
    return geometry_case("geometry D=%d %s%s" % (D, kind, " long" if long_preamble else ""), [toks], kind, D=D, first_match=npre)


def geometry_mixed(seed, kind, nbytes):
    """-> Case: 33000 random literals, then random (length, distance) pairs from the two grids with 0 to 3 literals between them until
    there are nbytes of output.  "fixed": one block; "dynamic": blocks of at most 30000 tokens, each with its own frequency_lengths"""
    rng = random.Random(seed)
    toks = [rng.randrange(256) for _ in range(33000)]
    n = len(toks)
    while n < nbytes:
        l, d, k = rng.choice(GEO_LENGTHS), rng.choice(GEO_DISTANCES), rng.randrange(4)
        toks.append((l, d))
        toks += [rng.randrange(256) for _ in range(k)]
        n += l + k
    blocks = [toks] if kind == "fixed" else [toks[i:i + 30000] for i in range(0, len(toks), 30000)]
    return geometry_case("geometry mixed %d %s" % (seed, kind), blocks, kind, first_match=33000)


def window_stats(case):
    """-> (the most matches whose codes begin within any 64 bits of the stream's body -- the tokens from the first match on --, the most
    output bytes of the tokens that begin within any 64 bits)"""
    body = [(p, t) for p, t in zip(case.token_pos, case.tokens)][case.first_match:]
    best_m = best_b = m = b = j = 0
    for i, (p, t) in enumerate(body):                      # a window of 64 bits that begins with token i
        while j < len(body) and body[j][0] < p + 64:
            m += 0 if isinstance(body[j][1], int) else 1
            b += 1 if isinstance(body[j][1], int) else body[j][1][0]
            j += 1
        best_m, best_b = max(best_m, m), max(best_b, b)
        m -= 0 if isinstance(t, int) else 1
        b -= 1 if isinstance(t, int) else t[0]
    return best_m, best_b


REJECTED_D = (1, 2, 113, 1537, 2049, 32768)
OBSIZE_D = (113, 512, 1537, 2049)


def geometry_rejected():
    """-> dict: reach [Case]: for D in REJECTED_D, both kinds, exactly D literals and then (258, D) -- the match reaches byte 0 and is
    valid --; short [Case]: D - 1 literals in front of it (not for D = 1): E_BAD_DISTANCE; obsize [Case]: for D in OBSIZE_D a stream
    whose only matches are (10, D), a literal, (10, D + 1), to be decoded with obsize in (D - 1, D, D + 1, 0): E_BAD_DISTANCE exactly
    for a non-zero obsize below D + 1"""
    reach, short, obs = [], [], []
    for D in REJECTED_D:
        rng = random.Random(100000 + D)
        lits = [rng.randrange(256) for _ in range(D)]
        for kind in GEO_KINDS:
            reach.append(geometry_case("reach D=%d %s" % (D, kind), [lits + [(258, D)]], kind, D=D, first_match=D))
            if D > 1:
                short.append(geometry_case("short D=%d %s" % (D, kind), [lits[1:] + [(258, D)]], kind, status=E_BAD_DISTANCE, D=D,
                                           first_match=D - 1))
    for k, D in enumerate(OBSIZE_D):
        rng = random.Random(200000 + D)
        lits = [rng.randrange(256) for _ in range(D + 5 + rng.randrange(64))]
        toks = lits + [(10, D), rng.randrange(256), (10, D + 1), rng.randrange(256)]
        obs.append(geometry_case("obsize D=%d" % D, [toks], GEO_KINDS[k & 1], D=D, first_match=len(lits)))
    return dict(reach=reach, short=short, obsize=obs)


@functools.lru_cache(None)
def geometry():
    """what both match-geometry test files run, built once per process -> dict: short, long [Case]: geometry_stream of every distance in
    both kinds (232 each: fixed, dynamic, fixed, ..), with the short and the long preamble; reach, short_by_one, obsize: geometry_rejected"""
    rej = geometry_rejected()
    return dict(short=[geometry_stream(D, kind) for D in GEO_DISTANCES for kind in GEO_KINDS],
                long=[geometry_stream(D, kind, True) for D in GEO_DISTANCES for kind in GEO_KINDS],
                reach=rej["reach"], short_by_one=rej["short"], obsize=rej["obsize"])


@functools.lru_cache(None)
def geometry_large():
    """-> (fixed, dynamic): the two mixed streams of 1 MiB"""
    return geometry_mixed(1, "fixed", 1 << 20), geometry_mixed(2, "dynamic", 1 << 20)


# ------------------------------------------------------------------------------------------------ the limits of the whole-GPU chains
# Streams that sit on each limit of hdlz_inflate_par.hip (k_par_*) and hdlz_inflate_any.hip (k_any_*): a case on the last value a chain
# takes and one on the first it gives up, with the verdict it must get (tests/chain_verdict.py reads it from the chains' control words).
# The sizes come from the constants in the kernels' sources (chain_verdict.source_constants, .lay); tests/test_chain_cases_cpu.py measures
# every declared property again from the case's own records and fails when a constant moves a case off its limit.
BULK_LL = (8,) * 226 + (9,) * 60                     # literals 0..225: 8 bits; 226..255, the end-of-block code and the lengths: 9 bits
BULK_DL = (4, 4) + (5,) * 28
WRITER_LL = (8,) * 255 + (9, 9)                      # literal v < 255: the eight bits of v, MSB first -- a run of literals WRITES chosen bits
EOB15_LL = (8,) * 255 + (9, 15, 10, 11, 12, 13, 14, 15)      # the end-of-block code has 15 bits
assert kraft(BULK_LL) == kraft(WRITER_LL) == kraft(EOB15_LL) == 1 << 15 and EOB15_LL[256] == 15
ONE_BIT_LL = tuple(sparse(257, {97: 1, 256: 1}))    # 'a' = the bit 0, end of block = the bit 1: a token per bit


def rev8(v):
    return int(format(v, "08b")[::-1], 2)


def header_image():
    """-> (bytes, header bits): a complete, valid, FINAL dynamic block -- 101 header bits, eight literals, the end-of-block code -- as
    whole bytes, none of them 255 (so that literals of WRITER_LL can write it)"""
    w = Bits()
    b = emit_block(w, list(ONE_BIT_LL), [0], [97] * 8, True)
    img = w.bytes()
    assert 255 not in img and zlib.decompressobj(-15).decompress(img) == b"a" * 8
    return img, b["span"][1]


def find_passes(z):
    """the bit positions of z that pass the two tests of k_any_find (BTYPE = 10, HLIT <= 29, HDIST <= 29; a complete code-length code),
    restated: what A_NCAND counts"""
    nbits, zp, out = 8 * len(z), z + bytes(16), []
    for B in range(2, len(z)):
        w = int.from_bytes(zp[B:B + 13], "little")
        for j in range(8):
            x = w >> j
            if 8 * B + j + 29 > nbits or (x >> 1) & 3 != 2 or (x >> 3) & 31 > 29 or (x >> 8) & 31 > 29:
                continue
            left, f = 128, x >> 17
            for _ in range(((x >> 13) & 15) + 4):
                left -= (128 >> (f & 7)) if f & 7 else 0
                f >>= 3
            if left == 0:
                out.append(8 * B + j)
    return out


class ChainCase(object):
    """name; z; plain (None: a damaged stream); expect: "any" | "fixed" | "serial", the verdict of the stream alone; evidence: for
    "serial", names of which at least one must show -- a W_* bit of A_WHY, "A_OVER", "C_NCROSS" (the fixed chain's list of end-of-block
    codes overflowed), "A_OPEN" (the gate stayed shut: the chain for any block types never ran); exactly / at_least: counters of the
    Verdict; props: the measured properties that put the case on its side of its limit; ndyn: its own dynamic blocks; images: the bit
    offsets in z of embedded header images; expect_at(lay): the verdict in a batch whose in_len gives the list sizes `lay`
    (chain_verdict.lay) -- the lists of the chain for any block types are sized by the CALL's in_len, so a case on one of those limits
    alone may be within it in a batch of longer streams; big: one of the two streams of 4 MiB"""

    def __init__(self, name, z, plain, expect, evidence=(), exactly=None, at_least=None, props=None, ndyn=0, images=(), expect_at=None,
                 big=False, records=()):
        self.name, self.z, self.plain, self.expect, self.evidence = name, z, plain, expect, tuple(evidence)
        self.exactly, self.at_least, self.props = exactly or {}, at_least or {}, props or {}
        self.ndyn, self.images, self.big, self.records = ndyn, tuple(images), big, list(records)
        self._expect_at = expect_at
        assert expect in ("any", "fixed", "serial") and (expect == "serial") == bool(evidence), name

    def expect_at(self, lay):
        return self._expect_at(lay) if self._expect_at else self.expect

    def __repr__(self):
        return "ChainCase(%s)" % self.name


class _Chain(object):
    """a stream under construction: the writer, the plain bytes, a record per block with its bit positions in z (the zlib header's 16 bits
    counted)"""

    def __init__(self, seed):
        self.w, self.out, self.rng, self.recs, self.ndyn, self.images = Bits(), bytearray(), random.Random(seed), [], 0, []

    @property
    def pos(self):
        return 16 + self.w.pos

    def dyn(self, ll, dl, toks, final=False, **kw):
        start = self.pos
        b = emit_block(self.w, list(ll), list(dl), toks, final, **kw)
        assert apply_tokens(self.out, toks) is not None
        self.ndyn += 1
        self.recs.append(dict(kind="dynamic", hdr=start, pay=16 + b["span"][1], eob=self.pos - ll[256], end=self.pos, ll=ll, dl=dl, tokens=toks, block=b))
        return self.recs[-1]

    def fixed(self, toks, final=False):
        start = self.pos
        emit_fixed_block(self.w, toks, final)
        assert apply_tokens(self.out, toks) is not None
        self.recs.append(dict(kind="fixed", hdr=start, pay=start + 3, eob=self.pos - 7, end=self.pos, ll=FIXED_LL, dl=FIXED_DL, tokens=toks))
        return self.recs[-1]

    def stored(self, data, final=False):
        start = self.pos
        self.w.put(1 if final else 0, 1)
        self.w.put(0, 2)
        if self.w.n:
            self.w.put(0, 8 - self.w.n)
        self.w.put(len(data), 16)
        self.w.put(len(data) ^ 0xFFFF, 16)
        assert self.w.n == 0 and len(data) <= 65535
        first = self.pos
        self.w.out += data
        self.w.pos += 8 * len(data)
        self.out += data
        self.recs.append(dict(kind="stored", hdr=start, data=first, length=len(data), end=self.pos))
        return self.recs[-1]

    def zseg(self, seg, data):
        """a raw-deflate segment made by zlib and closed with a full flush, at a byte boundary"""
        assert self.w.n == 0
        self.recs.append(dict(kind="zlib", hdr=self.pos, end=self.pos + 8 * len(seg)))
        self.w.out += seg
        self.w.pos += 8 * len(seg)
        self.out += data

    def lits(self, n8, n9=0, lo=226):
        """n8 random literals of 8 bits and n9 of 9 bits in BULK_LL (FIXED_LL: lo = 144), shuffled"""
        t = [self.rng.randrange(lo) for _ in range(n8)] + [self.rng.randrange(lo, 256) for _ in range(n9)]
        self.rng.shuffle(t)
        return t

    def bulk(self, ntok, final=False):
        """a block of BULK_LL: random literals and a few short matches"""
        toks, made = [], len(self.out)
        for _ in range(ntok):
            if made > 40 and self.rng.random() < 0.05:
                toks.append((self.rng.randint(3, 40), self.rng.randint(1, min(made, 3000))))
                made += toks[-1][0]
            else:
                toks.append(self.rng.randrange(256))
                made += 1
        return self.dyn(BULK_LL, BULK_DL, toks, final)

    def fill_to(self, target):
        """a block of BULK_LL, literals only, whose end-of-block code ends exactly at bit `target` of z"""
        T = target - self.pos - _hdr_bits(BULK_LL, BULK_DL) - BULK_LL[256]
        assert T >= 63, (target, self.pos)
        return self.dyn(BULK_LL, BULK_DL, self.lits((T - 9 * (T % 8)) // 8, T % 8))

    def next_at(self, residue, pb, ahead=0):
        """the first bit t that fill_to can reach with (t + ahead) % pb == residue"""
        t = self.pos + _hdr_bits(BULK_LL, BULK_DL) + BULK_LL[256] + 63
        return t + (residue - t - ahead) % pb

    def done(self, name, expect, **kw):
        z = wrap(self.w.bytes(), bytes(self.out))
        return ChainCase(name, z, bytes(self.out), expect, ndyn=self.ndyn, images=self.images, records=self.recs, **kw)


@functools.lru_cache(None)
def _hdr_bits(ll, dl):
    w = Bits()
    return emit_block(w, list(ll), list(dl), [], False)["span"][1]


def _payload_to(s, ll, lo9, pay, target):
    """literals of 8 bits (below lo9) and 9 bits that take the payload from bit `pay` exactly to bit `target`"""
    T = target - pay
    assert T >= 63
    t = [s.rng.randrange(lo9) for _ in range((T - 9 * (T % 8)) // 8)] + [s.rng.randrange(lo9, 256) for _ in range(T % 8)]
    s.rng.shuffle(t)
    assert sum(ll[v] for v in t) == T
    return t


def _tree_kinds():
    """the catalogue's kinds of tree as generators of (ll, dl, emit_block keywords) for block k"""
    def bits15(rng, k):
        return complete_code(286, rng, 15), complete_code(30, rng, 15), {}

    def cl7(rng, k):
        ll, dl = random_block_lengths(rng, count=40, max_len=9, dist_kind="several")
        return ll, dl, dict(ops=rle_ops(ll + dl), cl_lens=complete_code(19, rng, 7), hclen=19)

    def hlit257(rng, k):
        ll = [0] * 257
        for s_, l in zip([256] + rng.sample(range(256), 59), complete_code(60, rng, 9)):
            ll[s_] = l
        return ll, [1, 1], {}

    def hlit286(rng, k):
        ll = [0] * 286
        for s_, l in zip([256, 285] + rng.sample([v for v in range(285) if v != 256], 98), complete_code(100, rng, 12)):
            ll[s_] = l
        return ll, complete_code(30, rng, 9), {}

    def one_distance(rng, k):
        ll, _ = random_block_lengths(rng, count=80, max_len=11, dist_kind="one")
        c = (0, 3, 29, 12, 7)[k % 5]
        return ll, sparse(c + 1 + k % 2, {c: 1}), {}

    def no_distance(rng, k):
        ll, _ = random_block_lengths(rng, count=90, max_len=12, dist_kind="none")
        return ll, [0] * (1 + k % 3), {}

    def repeat_crosses(rng, k):
        a, b = rng.sample(range(256), 2)
        return sparse(260, {a: 2, b: 2, 256: 3, 257: 3, 258: 3, 259: 3}), [3] * 8, dict(rle=True)
    return (("15-bit codes", bits15), ("7-bit code-length code", cl7), ("HLIT 257", hlit257), ("HLIT 286", hlit286),
            ("one-code distance set", one_distance), ("empty distance set", no_distance), ("repeat crosses into the distances", repeat_crosses))


def _tree_cases(K):
    out = []
    for n, (name, gen) in enumerate(_tree_kinds()):
        s = _Chain(9100 + n)
        k = 0
        while True:
            last = k >= 2 and len(s.w.out) >= K["ANY_MIN"] + 300
            ll, dl, kw = gen(s.rng, k)
            r = s.dyn(ll, dl, tokens_for(s.rng, ll, dl, 1200, len(s.out)), last, **kw)
            b = r["block"]
            if name == "15-bit codes":
                assert b["max_ll"] == 15 and b["max_dl"] == 15
            elif name == "7-bit code-length code":
                assert b["max_cl"] == 7 and b["hclen"] == 19
            elif name.startswith("HLIT"):
                assert len(ll) == int(name[5:]) and (len(ll) == 257 or ll[285])
            elif name == "one-code distance set":
                assert b["ndcoded"] == 1
            elif name == "empty distance set":
                assert b["ndcoded"] == 0
            else:
                assert b["cross"] and b["rle"]
            k += 1
            if last:
                break
        out.append(s.done("trees: " + name, "any", at_least=dict(nblk=s.ndyn)))
    return out


def _position_stream(s, pb, tag):
    """into s: a block whose payload starts at bit = 0, 1 and pb - 1 mod pb, and one whose header's first bit is the last bit of a piece
    -> props"""
    props, H = {}, _hdr_bits(BULK_LL, BULK_DL)
    for what, residue in (("pay", 0), ("pay", 1), ("pay", pb - 1), ("hdr", pb - 1)):
        s.fill_to(s.next_at(residue, pb, H if what == "pay" else 0))
        r = s.bulk(700)
        props["%s %s = %d mod pb" % (tag, what, residue)] = (r[what], "pb", residue)
        assert r[what] % pb == residue
    return props


def _position_cases(K):
    out = []
    for what, residue in (("pay", 0), ("pay", 1), ("pay", 1023), ("hdr", 1023)):
        s = _Chain(9200 + residue + (what == "hdr"))
        s.bulk(1500)
        s.fill_to(s.next_at(residue, 1024, _hdr_bits(BULK_LL, BULK_DL) if what == "pay" else 0))
        r = s.bulk(1500)
        s.bulk(1500, True)
        out.append(s.done("position: %s at %d mod 1024" % ("payload" if what == "pay" else "header", residue), "any", at_least=dict(nblk=3),
                          props={"%s mod pb" % what: (r[what], "pb", residue)}))
    return out


def _eob_edge_cases(K):
    out = []
    for residue in (1023, 0):
        s = _Chain(9300 + residue)
        s.bulk(2200)
        pay = s.pos + _hdr_bits(EOB15_LL, (1, 1))
        target = pay + 4000 + (residue - (pay + 4000)) % 1024
        r = s.dyn(EOB15_LL, (1, 1), _payload_to(s, EOB15_LL, 255, pay, target))
        assert r["pay"] == pay and r["eob"] == target and r["end"] - r["eob"] == 15
        s.bulk(2200, True)
        out.append(s.done("end-of-block: a 15-bit code that starts at %d mod 1024" % residue, "any", at_least=dict(nblk=3),
                          props={"end-of-block code mod pb": (r["eob"], "pb", residue)}))
    return out


def _writer_block(s, nimg, lead, gap, tail, final=False):
    """a block of WRITER_LL whose literals write `nimg` header images into the stream, `gap` random literals (8 bits each) behind each"""
    img, _ = header_image()
    toks, at = [s.rng.randrange(255) for _ in range(lead)], []
    for _ in range(nimg):
        at.append(len(toks))
        toks += [rev8(v) for v in img] + [s.rng.randrange(255) for _ in range(gap)]
    toks += [s.rng.randrange(255) for _ in range(tail)]
    r = s.dyn(WRITER_LL, (0,), toks, final)
    s.images += [r["pay"] + 8 * k for k in at]
    return r


def _false_positive_cases(K):
    out = []
    for nimg in (1, 2, 3):
        s = _Chain(9400 + nimg)
        s.bulk(1500)
        r = _writer_block(s, nimg, 300, 512, 600)
        s.bulk(1500, True)
        taken = nimg < K["WALK_ROUNDS"]
        out.append(s.done("false positives: %d in a row inside one block" % nimg, "any" if taken else "serial",
                          evidence=() if taken else ("W_WALK_OWNER",), at_least=dict(nblk=3 + nimg, nreq=nimg if taken else 0),
                          props={"images in a row": (nimg, "WALK", ("below", "last", "first")[nimg - 1]),
                                 "whole pieces between the images and behind the last": (512 * 8 // 1024, "ONE", "above")}))
    # a request of more than REQ_MAX pieces: the rest is asked for in the next round
    s = _Chain(9410)
    s.bulk(1500)
    r = _writer_block(s, 1, 300, 0, (K["REQ_MAX"] + 16) * 128)
    s.bulk(1500, True)
    asked = -(-s.recs[-1]["pay"] // 1024) + (s.images[0] + header_image()[1]) // -1024        # from the image's first whole piece to the next block's payload
    c = s.done("false positives: a request longer than REQ_MAX pieces", "any", at_least=dict(nblk=4, nreq=2, reqp=K["REQ_MAX"] + 1),
               props={"pieces asked for": (asked, "REQ_MAX", "above"), "pieces asked for, of the list": (asked, "mapcap", "below")})
    out.append(c)
    return out


def _list_cases(K, lay):
    out = []
    img, _ = header_image()
    # ---- maxb: the true blocks and the images in a stored block together, one below the list's size, on it, one above
    for total in (63, 64, 65):
        s = _Chain(9500 + total)
        data = b"".join(img + bytes(64 - len(img)) for _ in range(total - 1)) + bytes(200)
        r = s.stored(data)
        s.images += [r["data"] + 512 * k for k in range(total - 1)]
        s.bulk(1500, True)
        c = s.done("lists: %d candidate blocks" % total, "any", exactly=dict(nblk=total))
        maxb = lay(len(c.z)).maxb
        c.props = {"candidate blocks": (total, "maxb", ("below", "last", "first")[total - 63])}
        if total > maxb:
            c.expect, c.evidence = "serial", ("A_OVER",)
        c._expect_at = lambda L, total=total: "any" if total <= L.maxb else "serial"
        out.append(c)
    # ---- candcap: a stored block of a four-byte period that passes k_any_find's tests (no position of it is a header), zero bytes
    # behind it that add to the list's size and not to the list
    period = (4 | 1 << 17 | 1 << 20).to_bytes(4, "little")           # BTYPE = 10, HLIT = HDIST = HCLEN = 0, the lengths 1, 1, 0, 0
    def build(m, zeros, seed=9600):
        s = _Chain(seed)
        s.stored(period * m + bytes(16 * zeros))
        s.bulk(1200, True)
        return s
    m = 1400
    while True:
        s = build(m, 0)
        z = wrap(s.w.bytes(), bytes(s.out))
        d = len(find_passes(z)) - lay(len(z)).candcap
        if d >= 2:
            break
        m += 40
    for over in (0, 1):
        s = build(m, d - over)
        c = s.done("lists: %s than candcap positions pass the search" % ("one more" if over else "no more"), "serial" if over else "any",
                   evidence=("A_OVER",) if over else ())
        n = len(find_passes(c.z))
        assert n == lay(len(c.z)).candcap + over, (n, lay(len(c.z)).candcap, over)
        c.exactly, c.props = dict(ncand=n), {"positions that pass the search": (n, "candcap", "first" if over else "last")}
        c._expect_at = lambda L, n=n: "any" if n <= L.candcap else "serial"
        out.append(c)
    return out


def _stored_cases(K, lay):
    out = []
    # ---- maxs: small non-empty stored blocks, a run of empty ones among them (they take no entry of the list)
    def build(n):
        s = _Chain(9700)
        for k in range(n):
            if k == n // 2:
                for _ in range(20):
                    s.stored(b"")
            s.stored(bytes((k * 7 + j) & 31 for j in range(16)), k == n - 1)
        return s
    n, want = 256, [0, 1]
    while want:
        s = build(n)
        zn = len(s.w.bytes()) + 6
        if n - lay(zn).maxs == want[0]:
            over = want.pop(0)
            c = s.done("stored: %s non-empty stored blocks than maxs" % ("one more" if over else "no more"), "serial" if over else "any",
                       evidence=("A_OVER",) if over else (), exactly=dict(ns=n, ncand=0), props={"non-empty stored blocks": (n, "maxs", "first" if over else "last")})
            assert len(c.z) == zn and not find_passes(c.z)
            c._expect_at = lambda L, n=n: "any" if n <= L.maxs else "serial"
            out.append(c)
        n += 1
        assert n < 400
    # ---- a final stored block whose data ends exactly at the trailer, its header at each bit offset
    for offset in range(8):
        s = _Chain(9710 + offset)
        s.bulk(1200)
        s.fill_to(s.next_at(0, 8))
        start = s.pos
        lits = emit_fixed_prefix(s.w, PREFIX_FOR_OFFSET[offset])
        s.out += lits
        s.recs.append(dict(kind="fixed", hdr=start, pay=start + 3, eob=s.pos - 7, end=s.pos, ll=FIXED_LL, dl=FIXED_DL, tokens=list(lits)))
        r = s.stored(bytes(s.rng.randrange(256) for _ in range(3000)), True)
        assert r["hdr"] % 8 == offset
        c = s.done("stored: the last block ends at the trailer, header at bit %d" % offset, "any", exactly=dict(ns=1),
                   props={"header bit": (r["hdr"], "byte", offset)})
        assert r["data"] // 8 + r["length"] == len(c.z) - 4
        out.append(c)
    return out


def fixed_walk_starts(pay, bits, pb):
    """where k_any_walk begins an item while it follows a fixed block whose payload starts at bit `pay` (bits: the tokens' sizes, the
    end-of-block code last): the payload's first bit, then the first token boundary at or behind every piece boundary"""
    starts, pos, limit = [pay], pay, (pay // pb + 1) * pb
    for nb in bits[:-1]:
        pos += nb
        if pos >= limit:
            starts.append(pos)
            limit = (pos // pb + 1) * pb
    return starts


def _fixed_cases(K):
    out = []
    F = K["FIX_MAX_BITS"]
    # ---- a fixed block behind a dynamic one, its payload on a piece boundary: the walk takes it while its end-of-block code starts within
    # FIX_MAX_BITS of the payload's first bit
    for over in (0, 1):
        s = _Chain(9800 + over)
        s.bulk(1500)
        s.fill_to(s.next_at(1024 - 3, 1024))
        pay = s.pos + 3
        r = s.fixed(_payload_to(s, FIXED_LL, 144, pay, pay + F - 1 + over))
        s.bulk(1500, True)
        starts = fixed_walk_starts(pay, token_bits(FIXED_LL, FIXED_DL, r["tokens"]) + [7], 1024)
        assert pay % 1024 == 0 and (max(starts) >= pay + F or r["eob"] >= max(starts) + 1024) == bool(over)
        out.append(s.done("fixed: a block of %d bits behind a dynamic one" % (r["end"] - r["hdr"]), "serial" if over else "any",
                          evidence=("W_WALK_FIX",) if over else (), at_least=dict(nblk=3),
                          props={"end-of-block code - payload": (r["eob"] - pay, "FIX", "first" if over else "last"), "payload mod pb": (pay, "pb", 0)}))
    # ---- a FIRST block that is fixed: the gate opens when its end-of-block code starts within FIRST_FIX_BITS and another type follows
    G = K["FIRST_FIX_BITS"]
    for over in (0, 1):
        for follow in ("dynamic", "stored"):
            s = _Chain(9810 + 2 * over + (follow == "stored"))
            r = s.fixed(_payload_to(s, FIXED_LL, 144, 19, 19 + G - 1 + over))
            assert r["pay"] == 19 and r["eob"] - 19 == G - 1 + over
            if follow == "dynamic":
                s.bulk(2200)
                s.bulk(2200, True)
            else:
                s.stored(bytes(s.rng.randrange(256) for _ in range(4200)), True)
            out.append(s.done("fixed first: its end-of-block code %d bits in, a %s block behind it" % (G - 1 + over, follow),
                              "serial" if over else "any", evidence=("A_OPEN",) if over else (),
                              exactly=dict(open=0 if over else 1), props={"end-of-block code - payload": (r["eob"] - 19, "FIRST_FIX", "first" if over else "last")}))
    s = _Chain(9820)
    s.fixed(s.lits(2400, 100, 144))
    s.fixed(s.lits(2400, 100, 144), True)
    out.append(s.done("fixed first: another fixed block behind it", "fixed", exactly=dict(open=0)))
    # ---- the fixed-block chain lists MAXCROSS end-of-block codes
    for over in (0, 1):
        s = _Chain(9830 + over)
        n = K["MAXCROSS"] + over
        for k in range(n):
            s.fixed([s.rng.randrange(144)] if k < n - 1 else [200], k == n - 1)
        assert (-s.w.pos) % 8 >= 3                     # (three zero bits behind the last end-of-block code: no fixed header, the chain of pieces ends)
        out.append(s.done("fixed chain: %d short fixed blocks" % n, "serial" if over else "fixed", evidence=("C_NCROSS",) if over else (),
                          props={"fixed blocks": (n, "MAXCROSS", "first" if over else "last")}))
    return out


def _token_cases(K, lay):
    out = []
    # ---- a token per bit: 1024 tokens in a piece, a list holds tcap.  One dense stretch ...
    s = _Chain(9900)
    s.bulk(1500)
    r = s.dyn(ONE_BIT_LL, (0,), [97] * (16 * 1024))
    s.bulk(1500, True)
    c = s.done("tokens: one stretch of 16 pieces with a token per bit", "any", at_least=dict(nblk=3, nx=3 + 1))
    L = lay(len(c.z))
    c.props = {"tokens per piece": (1024, "tcap", "above"), "lists wanted beyond the pieces' own": (3 * 16 + 8, "maxx", "below")}
    assert 1024 > L.tcap and 3 * 16 + 8 <= L.maxx
    out.append(c)
    # ... and a stream that is dense throughout: more lists than the budget of extra items (k_any_tokens: W_TCAP)
    s = _Chain(9901)
    b = emit_block(s.w, list(ONE_BIT_LL), [0], [], True, eob=False)
    n = 1000 * 1024
    s.w.put(0, n)
    s.w.put(1, 1)
    s.out += b"a" * n
    s.ndyn = 1
    s.recs.append(dict(kind="dynamic", hdr=16, pay=16 + b["span"][1], eob=s.pos - 1, end=s.pos, ll=ONE_BIT_LL, dl=(0,), tokens=None, ntokens=n))
    c = s.done("tokens: a token per bit throughout", "serial", evidence=("W_TCAP",), at_least=dict(nblk=1))
    want = lambda L: sum(-(-min(1024, s.recs[0]["eob"] - max(q * 1024, s.recs[0]["pay"])) // L.tcap) - 1
                         for q in range(s.recs[0]["pay"] // 1024, s.recs[0]["eob"] // 1024 + 1)) + 1
    L = lay(len(c.z))
    c.props = {"tokens per piece": (1024, "tcap", "above"), "lists wanted beyond the pieces' own": (want(L), "maxx", "above")}
    assert want(L) > L.maxx
    c._expect_at = lambda L_: "serial" if want(L_) > L_.maxx else "any"
    out.append(c)
    return out


@functools.lru_cache(None)
def _zlib_bulk():
    """-> (segment, data): 4.3 MB of raw deflate made by zlib (dynamic blocks of 6-bit random bytes), closed with a full flush"""
    import numpy as np
    data = np.random.default_rng(77).integers(0, 64, 5900000, dtype=np.uint8).tobytes()
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    seg = co.compress(data) + co.flush(zlib.Z_FULL_FLUSH)
    assert len(seg) >= (4 << 20) + 4096 and (seg[0] >> 1) & 3 == 2
    return seg, data


def _big_cases(K, lay):
    seg, data = _zlib_bulk()
    s = _Chain(9950)
    s.zseg(seg, data)
    props = _position_stream(s, 2048, "behind 4 MiB:")
    s.bulk(1500, True)
    a = s.done("pb = 2048: positions of headers and payloads", "any", at_least=dict(nblk=s.ndyn), props=props, big=True)
    s = _Chain(9951)
    s.zseg(seg, data)
    s.bulk(1500)
    r = _writer_block(s, 2, 600, 2048, 2048)
    s.bulk(1500, True)
    b = s.done("pb = 2048: two false positives in a row", "any", at_least=dict(nblk=s.ndyn + 2, nreq=2), big=True,
               props={"images in a row": (2, "WALK", "last"), "whole pieces between the images and behind the last": (2048 * 8 // 2048, "ONE", "above")})
    for c in (a, b):
        assert lay(len(c.z)).pb == 2048
    return [a, b]


def _damaged(case, rec, what):
    """-> ChainCase: `case` with one bit flipped -- "header": BTYPE 10 -> 11 in the block of `rec`; "payload": the first bit behind the
    payload's 200th after which stock zlib no longer finds the stream's end"""
    z = bytearray(case.z)
    if what == "header":
        bit = rec["hdr"] + 1
    else:
        for bit in range(rec["pay"] + 200, rec["eob"]):
            m = bytearray(case.z)
            m[bit >> 3] ^= 1 << (bit & 7)
            d = zlib.decompressobj(-15)                  # (the raw stream: a flip that only changes a literal is no damage to a decoder)
            try:
                d.decompress(bytes(m[2:]))
                bad = not d.eof
            except zlib.error:
                bad = True
            if bad:
                break
        else:
            raise AssertionError("no flip found")
    z[bit >> 3] ^= 1 << (bit & 7)
    c = ChainCase("damaged (%s): %s" % (what, case.name), bytes(z), None, "serial", evidence=("damaged",))
    c.neighbour, c.bit = case, bit
    return c


def chain_limits(K, L):
    """the largest value each limit of the chains TAKES, from the constants K (chain_verdict.source_constants) and the list sizes L
    (chain_verdict.lay of the stream's length) -- and the two moduli of the position properties"""
    return dict(pb=L.pb, byte=8, ONE=1, FIX=K["FIX_MAX_BITS"] - 1, FIRST_FIX=K["FIRST_FIX_BITS"] - 1, WALK=K["WALK_ROUNDS"] - 1,
                MAXCROSS=K["MAXCROSS"], REQ_MAX=K["REQ_MAX"], maxb=L.maxb, maxs=L.maxs, candcap=L.candcap, mapcap=L.mapcap, tcap=L.tcap, maxx=L.maxx)


def off_limit(case, K, L):
    """the declared properties of `case` that do not hold under the constants K and list sizes L -> [text]: (measured, limit, side) with
    side "last" (the largest value taken), "first" (one more), "below", "above", or a residue of a bit position modulo the limit"""
    lim, out = chain_limits(K, L), []
    for what, (m, key, side) in sorted(case.props.items()):
        v = lim[key]
        ok = m % v == side if isinstance(side, int) else {"last": m == v, "first": m == v + 1, "below": m < v, "above": m > v}[side]
        if not ok:
            out.append("%s: %s = %d is not %s %s = %d" % (case.name, what, m, "%d modulo" % side if isinstance(side, int) else side, key, v))
    return out


@functools.lru_cache(None)
def chain_cases():
    """-> [ChainCase]: every limit of the two whole-GPU inflate chains, the last value taken and the first given up"""
    import chain_verdict as V
    K = V.source_constants()
    cs = _tree_cases(K) + _position_cases(K) + _eob_edge_cases(K) + _false_positive_cases(K) + _list_cases(K, V.lay) + \
        _stored_cases(K, V.lay) + _fixed_cases(K) + _token_cases(K, V.lay) + _big_cases(K, V.lay)
    by = dict((c.name, c) for c in cs)
    a, b = by["position: payload at 0 mod 1024"], by["end-of-block: a 15-bit code that starts at 1023 mod 1024"]
    cs += [_damaged(a, a.records[2], "header"), _damaged(b, b.records[1], "payload")]
    assert len(set(c.name for c in cs)) == len(cs)
    for c in cs:
        assert len(c.z) >= K["ANY_MIN"], c.name
    return cs
