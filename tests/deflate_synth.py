"""Composer of hand-built DEFLATE streams (pure Python, no torch).

Every stream is assembled block by block from an explicit plan: code lengths
are chosen (random Kraft-complete trees of a given shape), not derived from
symbol frequencies, and the tokens are a program over those codes that uses
every coded symbol it can.  The composer writes the output as it goes, so each
valid case carries its own expected bytes.

Beyond what encoders write, the corpus holds what only the reference decoder
accepts (lib/deflate_decompress.c:555-628, :799-853; decompress_template.h:
99-105): litlen symbols 286/287 and offset symbols 30/31 in use, HLIT up to
288 and HDIST up to 32, a single codeword of length 1 read from a '1' bit, an
empty offset code whose matches read distance symbol 0 from one bit.  Such a
case is marked ref_only: zlib refuses it.

corpus() returns the cases; each has tags for the coverage gate (TAGS lists
every tag that must be reached).  Everything comes from fixed seeds.
"""
import random
import zlib

from tests import deflate_audit as A
from tests.streams import BitWriter

# symbol -> base / extra bits with the reference's aliases: 286, 287 mean
# length 258; offset symbols 30, 31 mean what 29 means
LBASE = A.LEN_BASE + [258, 258]
LEXTRA = A.LEN_EXTRA + [0, 0]
DBASE = A.DIST_BASE + [24577, 24577]
DEXTRA = A.DIST_EXTRA + [13, 13]
PERM = A.PERM

LIT_SHAPES = ("flat", "steep", "tail", "edge", "random")
TB_BIG = 8192        # bytes of input behind a header for the larger tables

TAGS = ([f"lit:cw{n}" for n in range(1, 16)] + [f"off:cw{n}" for n in range(1, 16)] +
        [f"len{s}:{e}" for s in range(257, 288) for e in ("lo", "hi")] +
        [f"dist{s}:{e}" for s in range(32) for e in ("lo", "hi")] +
        [f"stored@bit{b}:{n}" for b in range(8) for n in (0, 1, 65535)] +
        [f"pre:{s}-{e}" for s in (16, 17, 18) for e in ("min", "max", "across")] +
        [f"shape:{s}" for s in LIT_SHAPES] +
        [f"tb-{b}:lit:cw{n}" for b in ("big", "small") for n in (9, 10, 11)] +
        [f"tb-{b}:off:cw{n}" for b in ("big", "small") for n in (7, 8, 9)] +
        ["lit:sym286", "lit:sym287", "off:sym30", "off:sym31", "hlit:288", "hdist:32",
         "single-cw-bit0", "single-cw-bit1", "single-cw-lit", "empty-off", "empty-off-match",
         "258-as-284", "258-as-285", "dist:1", "dist:32768", "overlap", "dist-to-start",
         "dict-to-start", "unused-cw", "hdr-untrimmed", "hclen:19", "hclen:5", "static",
         "tiny-blocks", "tb:8191", "tb:8192", "tb:8193", "tb:prev-small", "tb:prev-big",
         "long-block", "multi-block", "zlib", "gzip", "gzip-members", "dict-raw", "dict-zlib",
         "bad:oversub-lit", "bad:oversub-off", "bad:oversub-pre", "bad:incomplete-lit",
         "bad:incomplete-off", "bad:incomplete-pre", "bad:single-cw-len2", "bad:pre16-first",
         "bad:pre-overshoot", "bad:stored-nlen", "bad:dist-beyond", "bad:dict-beyond",
         "bad:btype3", "bad:no-eob", "bad:short-1", "bad:dictid", "bad:footer"] +
        [f"bad:trunc{k}" for k in range(1, 13)])


def _rev(v, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def codes(lens):
    """LSB-first codewords ready for BitWriter.put: [(bits, len) or None]"""
    return [None if c is None else (_rev(c, n), n)
            for c, n in zip(A.canonical_codes(lens), lens)]


def tree_lengths(rng, n, maxlen, weight):
    """n codeword lengths of a complete code: leaves of a random binary tree,
    grown by splitting a leaf chosen with probability weight(depth)"""
    if n == 1:
        return [1]
    leaves = [1, 1]
    while len(leaves) < n:
        cand = [i for i, d in enumerate(leaves) if d < maxlen]
        i = rng.choices(cand, [weight(leaves[i]) for i in cand])[0]
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    return leaves


def shape_weight(shape, edge=(8, 9, 10)):
    """flat: the shallowest leaf splits; steep: the deepest (lengths 1..15);
    tail: most leaves end at 12..15; edge: many at edge+1 (both sides of the
    table sizes); random"""
    if shape == "flat":
        return lambda d: 1e-6 ** d
    if shape == "steep":
        return lambda d: 1e3 ** d
    if shape == "tail":
        return lambda d: 100.0 if d >= 11 else 1.0
    if shape == "edge":
        return lambda d: 100.0 if d in edge else (1.0 if d < edge[0] else 0.01)
    return lambda d: 1.0


class Case:
    """one stream: fmt, data, avail (the output space to give), out (the
    composer's bytes for a valid case, else None), tags, ref_only, and the
    preset dictionary (b"" for none)"""

    def __init__(self, name, fmt, data, out, tags, ref_only=False, avail=None,
                 dictionary=b"", ordinary=False):
        self.name, self.fmt, self.data, self.out = name, fmt, data, out
        self.tags, self.ref_only, self.dictionary = set(tags), ref_only, dictionary
        self.avail = avail if avail is not None else len(out)
        self.valid = out is not None
        self.ordinary = ordinary

    def __repr__(self):
        return f"Case({self.name}, {self.fmt}, {len(self.data)} B)"


class Composer:
    """a raw DEFLATE stream under construction; hist is the window the
    distances may reach (the dictionary, then the output)"""

    def __init__(self, seed, dictionary=b""):
        self.rng = random.Random(seed)
        self.w = BitWriter()
        self.hist = bytearray(dictionary[-32768:])
        self.base = len(self.hist)
        self.tags = set()
        self.ref_only = False
        self.ordinary = True
        self.prev_huff = False
        self.blocks = []    # (start bit, type, litlen / offset lengths used)

    @property
    def out(self):
        return bytes(self.hist[self.base:])

    def bits(self):
        return 8 * len(self.w.out) + self.w.n

    def finish(self, pad=b""):
        return self.w.finish() + pad

    # ---------------------------------------------------------- blocks
    def stored(self, data, final=0, nlen_xor=0):
        if self.prev_huff:
            self.tags.add(f"stored@bit{self.w.n}:{len(data)}")
        self.prev_huff = False
        self.blocks.append((self.bits(), 0, (), ()))
        w = self.w
        w.put(final, 1)
        w.put(0, 2)
        w.finish()
        n = len(data)
        nlen = (n ^ 0xFFFF) ^ nlen_xor
        w.out += bytes([n & 255, n >> 8, nlen & 255, nlen >> 8])
        w.out += data
        self.hist += data
        if nlen_xor:
            self.tags.add("bad:stored-nlen")

    def _tokens(self, nbytes, lit_use, len_use, d_use, ll, dl):
        """a token program of about nbytes of output: every usable symbol
        once while it can be, then random ones; extra bits at their extremes
        as often as in between"""
        rng, hist, tags = self.rng, self.hist, self.tags
        toks = []
        pending = set(lit_use) | set(len_use)
        dpend = set(d_use)
        allsym = sorted(set(lit_use) | set(len_use))
        end = len(hist) + nbytes
        while len(hist) < end:
            room = end - len(hist)
            s = rng.choice(sorted(pending)) if pending and rng.random() < 0.7 \
                else rng.choice(allsym)
            ds = None
            if s >= 257:
                reach = [d for d in d_use if DBASE[d] <= len(hist)]
                if LBASE[s - 257] > room or not reach:
                    s = None
                else:
                    dp = [d for d in reach if d in dpend]
                    ds = rng.choice(dp) if dp and rng.random() < 0.8 else rng.choice(reach)
            if s is None:
                if not lit_use:
                    break
                s = rng.choice(lit_use)
            pending.discard(s)
            if s < 256:
                toks.append((s,))
                hist.append(s)
                tags.add(f"lit:cw{ll[s]}")
                continue
            dpend.discard(ds)
            xb = LEXTRA[s - 257]
            lx = self._extreme(xb, room - LBASE[s - 257])
            length = LBASE[s - 257] + lx
            dxb = DEXTRA[ds]
            dx = self._extreme(dxb, len(hist) - DBASE[ds])
            dist = DBASE[ds] + dx
            self._tag_match(s, lx, xb, ds, dx, dxb, length, dist, ll, dl)
            toks.append((s, lx, ds, dx))
            if dist >= length:
                hist += hist[-dist:len(hist) - dist + length]
            else:
                seg = hist[-dist:]
                hist += (seg * (length // dist + 1))[:length]
        return toks

    def _extreme(self, xb, cap):
        m = min((1 << xb) - 1, cap)
        r = self.rng.random()
        return m if r < 0.35 else 0 if r < 0.7 else self.rng.randint(0, m)

    def _tag_match(self, s, lx, xb, ds, dx, dxb, length, dist, ll, dl):
        t = self.tags
        t.add(f"lit:cw{ll[s]}")
        if dl is not None:
            t.add(f"off:cw{dl[ds]}")
        if lx == 0:
            t.add(f"len{s}:lo")
        if lx == (1 << xb) - 1:
            t.add(f"len{s}:hi")
        if dx == 0:
            t.add(f"dist{ds}:lo")
        if dx == (1 << dxb) - 1:
            t.add(f"dist{ds}:hi")
        if s == 284 and lx == 31:
            t.add("258-as-284")
        if s == 285:
            t.add("258-as-285")
        if s >= 286:
            t.add(f"lit:sym{s}")
            self.ref_only = True
        if ds >= 30:
            t.add(f"off:sym{ds}")
            self.ref_only = True
        if dist == 1:
            t.add("dist:1")
        if dist == 32768:
            t.add("dist:32768")
        if dist < length:
            t.add("overlap")
        if dist == len(self.hist):
            t.add("dict-to-start" if self.base else "dist-to-start")

    def _put_tokens(self, toks, lc, dc, dbit=None):
        """dbit "alt": a single-codeword or empty offset code, whose one-bit
        distance codewords are written as 0, 1, 0, ... (None: the canonical
        codes).  -> how many 0 and 1 bits were written that way"""
        put = self.w.put
        nbit = [0, 0]
        for t in toks:
            put(*lc[t[0]])
            if len(t) == 1:
                continue
            s, lx, ds, dx = t
            put(lx, LEXTRA[s - 257])
            if dbit is None:
                put(*dc[ds])
            else:
                b = (nbit[0] + nbit[1]) & 1
                nbit[b] += 1
                put(b, 1)
            put(dx, DEXTRA[ds])
        return nbit

    def static(self, nbytes, final=0, end_bit=None, lit_use=None, len_use=None, d_use=None,
               bad_dist=False):
        """a static block; end_bit: pad with 9-bit literals so that the block
        ends at that bit of a byte; bad_dist: end with a match one byte beyond
        the window"""
        self.tags.add("static")
        ll, dl = A.STATIC_LL, A.STATIC_D
        lit_use = lit_use if lit_use is not None else list(range(256))
        toks = self._tokens(nbytes, lit_use, len_use if len_use is not None else
                            list(range(257, 286)), d_use if d_use is not None else
                            list(range(30)), ll, dl)
        w = self.w
        self.blocks.append((self.bits(), 1, (), ()))
        w.put(final, 1)
        w.put(1, 2)
        lc, dc = codes(ll), codes(dl)
        self._put_tokens(toks, lc, dc)
        if bad_dist:
            n = len(self.hist) + 1
            ds = A.dist_sym(n) if n <= 32768 else 29
            w.put(*lc[257])
            w.put(*dc[ds])
            w.put(n - DBASE[ds], DEXTRA[ds])
            self.tags.add("bad:dict-beyond" if self.base else "bad:dist-beyond")
        if end_bit is not None:
            while (w.n + 7) % 8 != end_bit:
                c = self.rng.randrange(144, 256)
                w.put(*lc[c])
                self.hist.append(c)
        w.put(*lc[256])
        self.prev_huff = True

    def dynamic(self, nbytes, final=0, lit_shape="random", off_shape="random", n_lit=None,
                len_use=None, d_use=None, unused=0, hlit_pad=0, hdist_pad=0, hclen19=False,
                rle="random", lit_code=None, off_code=None, cross16=False, mutate=None):
        """a dynamic block.  lit_code: None (a tree of lit_shape over n_lit
        literals, the length symbols len_use and EOB), "eob-only" (a single
        codeword: the block is empty), "no-eob".  off_code: None (a tree of
        off_shape over d_use), "empty", "single" (one codeword of length 1).
        unused: that many extra symbols get lengths and are never used.
        mutate(stage, obj) may damage the lengths ("lens"), the precode items
        ("items") or the precode lengths ("pre")."""
        rng, tags = self.rng, self.tags
        tags.add(f"shape:{lit_shape}")
        reach = len(self.hist) + nbytes
        if len_use is None:
            len_use = list(range(257, 286))
        if d_use is None:
            d_use = [d for d in range(30) if DBASE[d] <= max(reach // 2, 1)]
        n_lit = n_lit if n_lit is not None else rng.randint(8, 200)
        lit_use = sorted(rng.sample(range(256), n_lit))
        ll, dl = [0] * 288, [0] * 32
        if lit_code == "eob-only":
            ll[256] = 1
            lit_use, len_use, nbytes = [], [], 0
            tags.add("single-cw-lit")
            self.ordinary = False
        else:
            syms = lit_use + len_use + ([] if lit_code == "no-eob" else [256])
            spare = [s for s in range(256) if s not in lit_use]
            syms += rng.sample(spare, min(unused, len(spare)))
            for s, n in zip(syms, tree_lengths(rng, len(syms), 15,
                                               shape_weight(lit_shape, (8, 9, 10)))):
                ll[s] = n
        dbit = None
        if off_code == "empty":
            d_use = [0]
            tags.add("empty-off")
        elif off_code == "single":
            ds = d_use[0] if d_use else 0
            dl[ds] = 1
            d_use = [ds]
        else:
            dsyms = list(d_use)
            spare = [d for d in range(30) if d not in dsyms]
            dsyms += rng.sample(spare, min(unused, len(spare)))
            if len(dsyms) == 1:
                dsyms.append(rng.choice(spare))
            for s, n in zip(dsyms, tree_lengths(rng, len(dsyms), 15,
                                                shape_weight(off_shape, (6, 7, 8)))):
                dl[s] = n
        if unused:
            tags.add("unused-cw")
        lc0, dc0 = codes(ll), codes(dl)
        toks = self._tokens(nbytes, lit_use, len_use, d_use, ll,
                            None if off_code in ("empty", "single") else dl)
        if off_code in ("empty", "single") and any(len(t) > 1 for t in toks):
            dbit = "alt"
        if mutate:
            mutate("lens", (ll, dl))
        hlit, hdist = A.trimmed_counts(ll, dl)
        if lit_code == "no-eob" or ll[256] == 0:
            tags.add("bad:no-eob")
        hlit, hdist = min(288, hlit + hlit_pad), min(32, hdist + hdist_pad)
        if hlit_pad or hdist_pad:
            tags.add("hdr-untrimmed")
            self.ordinary = False
        if cross16:
            v = dl[0]
            if v and dl[1] == v and dl[2] == v and v in ll[:hlit - 1]:
                j = ll.index(v)
                ll[j], ll[hlit - 1] = ll[hlit - 1], ll[j]
                lc0 = codes(ll)
        if hlit > 286:
            tags.add(f"hlit:{hlit}")
            self.ref_only = True
        if hdist > 30:
            tags.add(f"hdist:{hdist}")
            self.ref_only = True
        seq = ll[:hlit] + dl[:hdist]
        items = A.precode_items_ref(seq) if rle == "greedy" else self._rle(seq)
        if mutate:
            mutate("items", items)
        self._tag_items(items, hlit)
        used = sorted({s for s, _ in items})
        if len(used) == 1:
            used.append(next(s for s in (18, 0, 8) if s not in used))
        pre = [0] * 19
        for s, n in zip(used, tree_lengths(rng, len(used), 7, shape_weight("random"))):
            pre[s] = n
        if mutate:
            mutate("pre", pre)
        hclen = 19 if hclen19 else A.trimmed_hclen(pre)
        if hclen19 and A.trimmed_hclen(pre) < 19:
            tags.add("hclen:19")
        if hclen == 5:
            tags.add("hclen:5")
        w = self.w
        self.blocks.append((self.bits(), 2, {ll[t[0]] for t in toks} | {ll[256]},
                            set() if dbit else {dl[t[2]] for t in toks if len(t) > 1}))
        w.put(final, 1)
        w.put(2, 2)
        w.put(hlit - 257, 5)
        w.put(hdist - 1, 5)
        w.put(hclen - 4, 4)
        for i in range(hclen):
            w.put(pre[PERM[i]], 3)
        pc = codes(pre)
        for s, r in items:
            w.put(*(pc[s] or (0, 1)))
            if s >= 16:
                w.put(r - (11 if s == 18 else 3), A.PRE_EXTRA[s])
        nbit = self._put_tokens(toks, lc0, dc0, dbit)
        if lit_code == "eob-only":
            b = 1 if self.rng.random() < 0.5 else 0
            w.put(b, 1)
            tags.add(f"single-cw-bit{b}")
            if b:
                self.ref_only = True
        elif lc0[256] is not None:
            w.put(*lc0[256])
        self.prev_huff = True
        if dbit and off_code == "empty":
            tags.add("empty-off-match")
            self.ref_only = True
        elif dbit:
            tags |= {"off:cw1", "single-cw-bit0"}
            if nbit[1]:
                tags.add("single-cw-bit1")
                self.ref_only = True
        return toks

    def table_tags(self, in_n):
        """which dynamic blocks get the kernels' larger tables (the rule of
        inflate_kernel.hip: the previous block was not under TB_BIG bytes of
        input, and TB_BIG bytes of input are left at the header), and which
        codeword lengths around the table sizes they used"""
        prev = None
        for at, btype, lset, oset in self.blocks:
            was_small = prev is not None and at != 0 and at - prev < 8 * TB_BIG
            prev = at
            if btype != 2:
                continue
            side = "big" if not was_small and in_n - at // 8 >= TB_BIG else "small"
            self.tags.update(f"tb-{side}:lit:cw{n}" for n in set(lset) & {9, 10, 11})
            self.tags.update(f"tb-{side}:off:cw{n}" for n in set(oset) & {7, 8, 9})

    def _rle(self, seq):
        """random run-length items: 16/17/18 runs of minimum, maximum and
        in-between counts, and plain lengths"""
        rng, items, i, n = self.rng, [], 0, len(seq)
        while i < n:
            v, j = seq[i], i
            while j < n and seq[j] == v:
                j += 1
            left = j - i
            p = rng.random()
            if v == 0 and left >= 11 and p < 0.7:
                m = min(left, 138)
                r = rng.choice([11, m, rng.randint(11, m)])
                items.append((18, r))
            elif v == 0 and left >= 3 and p < 0.7:
                m = min(left, 10)
                r = rng.choice([3, m, rng.randint(3, m)])
                items.append((17, r))
            elif v and i and seq[i - 1] == v and left >= 3 and p < 0.8:
                m = min(left, 6)
                r = rng.choice([3, m, rng.randint(3, m)])
                items.append((16, r))
            else:
                r = 1
                items.append((v, None))
            i += r
        return items

    def _tag_items(self, items, hlit):
        i = 0
        for s, r in items:
            if s >= 16:
                lo, hi = (11, 138) if s == 18 else (3, 6 if s == 16 else 10)
                if r == lo:
                    self.tags.add(f"pre:{s}-min")
                if r == hi:
                    self.tags.add(f"pre:{s}-max")
                if i < hlit < i + r:
                    self.tags.add(f"pre:{s}-across")
            i += r or 1


# ------------------------------------------------------------- wrappers

def zlib_wrap(raw, out, dictionary=None):
    if dictionary is None:
        return b"\x78\x9c" + raw + zlib.adler32(out).to_bytes(4, "big")
    flg = 0x20 | 0x80
    flg |= 31 - ((0x78 << 8 | flg) % 31)
    return (bytes([0x78, flg]) + zlib.adler32(dictionary).to_bytes(4, "big") + raw +
            zlib.adler32(out).to_bytes(4, "big"))


def gzip_wrap(raw, out):
    return (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw +
            zlib.crc32(out).to_bytes(4, "little") +
            (len(out) & 0xFFFFFFFF).to_bytes(4, "little"))


def stored_prefix(dictionary):
    """one non-final stored block holding the window a dictionary gives:
    decoding prefix + raw body without a dictionary is decoding the body with
    it (the rule of libdeflate_amd.h for raw DEFLATE)"""
    win = dictionary[-32768:]
    n = len(win)
    return b"\x00" + bytes([n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + win, n


def dict_verdict(dec, case, out_avail, want_actual_out=True):
    """(result, actual_in, actual_out, bytes) of a dictionary case from a
    decoder without a dictionary API (oracle or reference), through the
    stored prefix"""
    pre, n = stored_prefix(case.dictionary)
    raw, extra = case.data, 0
    if case.fmt == "zlib":
        hdr = raw[:6]
        if (hdr[1] & 0x20) == 0 or int.from_bytes(hdr[2:6], "big") != zlib.adler32(case.dictionary):
            return (1, 0, 0, b"")
        raw, extra = raw[6:], 10
    r, ain, aout, out = dec.decompress_ex("deflate", pre + raw, out_avail + n, want_actual_out)
    if r != 0:
        return (r, 0, 0, b"")
    out = out[n:]
    ain -= len(pre)
    aout = aout - n if want_actual_out else 0
    if case.fmt == "zlib":
        if len(raw) < ain + 4 or raw[ain:ain + 4] != zlib.adler32(out).to_bytes(4, "big"):
            return (1, 0, 0, b"")
        ain += extra
    return (r, ain, aout, out)


# --------------------------------------------------------------- corpus

def _case(name, c, tags=(), fmt="deflate", pad=b"", avail=None, valid=True):
    raw = c.finish(pad)
    c.table_tags(len(raw))
    out = c.out if valid else None
    t = set(c.tags) | set(tags)
    if not valid:
        avail = avail if avail is not None else len(c.out) + 64
    return Case(name, fmt, raw, out, t, c.ref_only and valid, avail,
                ordinary=c.ordinary and valid)


def _ref_only_cases():
    """one small case per behaviour zlib refuses"""
    cs = []
    c = Composer(0x5E0001)
    c.static(300)
    c.dynamic(2000, final=1, len_use=list(range(257, 288)), lit_shape="random")
    cs.append(_case("sym286-287", c))
    c = Composer(0x5E0002)
    c.static(30000, d_use=list(range(30)))
    c.dynamic(6000, final=1, d_use=[0, 3, 29, 30, 31], hlit_pad=0)
    cs.append(_case("off30-31", c))
    c = Composer(0x5E0003)
    c.dynamic(3000, hlit_pad=40, hdist_pad=40)
    c.dynamic(500, final=1)
    cs.append(_case("hlit288-hdist32", c))
    for k in range(4):
        c = Composer(0x5E0010 + k)
        c.dynamic(400)
        c.dynamic(0, lit_code="eob-only", off_code="empty")
        c.dynamic(900, off_code="single", d_use=[k * 3])
        c.dynamic(700, off_code="empty", final=1)
        cs.append(_case(f"incomplete{k}", c))
    return cs


def _plain_cases():
    cs = []
    # every shape, both table sizes' sides of the lengths
    for i, (ls, os_) in enumerate([(s, o) for s in LIT_SHAPES for o in LIT_SHAPES]):
        c = Composer(0x5E0100 + i)
        c.dynamic(6000 + 997 * i, final=0, lit_shape=ls, off_shape=os_, n_lit=60 + 8 * i,
                  unused=i % 3 * 5, rle="greedy" if i % 4 == 0 else "random",
                  cross16=i % 2 == 1, hclen19=i % 5 == 0)
        c.dynamic(3000, final=1, lit_shape=LIT_SHAPES[(i + 2) % 5], off_shape="steep")
        cs.append(_case(f"shape-{ls}-{os_}", c))
    # a litlen code of 256 lengths of 8: HCLEN 5 (presyms 16, 17, 18, 0, 8)
    c = Composer(0x5E0180)
    c.static(1000)
    c.dynamic(5000, final=1, lit_shape="flat", n_lit=255, len_use=[], off_code="empty",
              rle="greedy")
    cs.append(_case("flat8", c))
    # stored blocks of 0, 1 and 65535 bytes after a Huffman block ending on
    # each bit of a byte
    for b in range(8):
        for n in (0, 1, 65535):
            c = Composer(0x5E0200 + 8 * b + n % 7)
            c.static(50 + b, end_bit=b)
            c.stored(bytes(c.rng.randrange(256) for _ in range(n)) if n < 100 else
                     random.Random(b).randbytes(n))
            c.static(20, final=1)
            cs.append(_case(f"stored@bit{b}:{n}", c))
    # zero runs from the litlen lengths into the offset lengths
    for k in range(3):
        c = Composer(0x5E0190 + k)
        c.dynamic(20000, len_use=list(range(257, 270 + k)), hlit_pad=1 + 7 * k,
                  d_use=list(range(4 + k, 20)), rle="greedy" if k < 2 else "random")
        c.dynamic(2000, final=1)
        cs.append(_case(f"zero-runs-across{k}", c))
    # many tiny blocks of every type
    c = Composer(0x5E0300)
    for k in range(240):
        r = c.rng.random()
        if r < 0.3:
            c.stored(bytes(c.rng.randrange(256) for _ in range(c.rng.randrange(4))))
        elif r < 0.6:
            c.static(c.rng.randrange(6))
        else:
            c.dynamic(c.rng.randrange(6), n_lit=c.rng.randint(1, 8))
    c.static(3, final=1)
    c.tags.add("tiny-blocks")
    cs.append(_case("tiny-blocks", c))
    # the first header with 8191, 8192, 8193 bytes of input behind it; a
    # second block behind a first one just under / over 8 KiB
    for n in (8191, 8192, 8193):
        c = Composer(0x5E0400 + n)
        c.dynamic(7000, final=1, lit_shape="edge", off_shape="edge", n_lit=240)
        raw = c.finish()
        assert len(raw) < n, len(raw)
        c.table_tags(n)
        cs.append(Case(f"tb:{n}", "deflate", raw + bytes(n - len(raw)), c.out,
                       c.tags | {f"tb:{n}"}, ordinary=True))
    for k, target in enumerate((8 * TB_BIG - 48, 8 * TB_BIG - 16, 8 * TB_BIG + 16,
                                8 * TB_BIG + 48)):
        nb = target // 8
        for _ in range(4):
            c = Composer(0x5E0420 + k)
            c.dynamic(nb, lit_shape="edge", off_shape="edge", n_lit=230)
            nb = max(1, nb * target // max(c.bits(), 1))
        small = c.bits() < 8 * TB_BIG
        c.dynamic(40000, final=1, lit_shape="edge", off_shape="edge", n_lit=230)
        c.tags.add("tb:prev-small" if small else "tb:prev-big")
        cs.append(_case(f"tb-prev{k}", c))
    return cs


def _long_cases():
    cs = []
    for i, n in enumerate((65536, 262144, 1 << 20)):
        c = Composer(0x5E0500 + i)
        c.dynamic(n, final=1, lit_shape=LIT_SHAPES[i], off_shape="edge", n_lit=100,
                  d_use=list(range(30)))
        c.tags.add("long-block")
        cs.append(_case(f"long{n}", c))
    for i, total in enumerate((1 << 20, 2 << 20, 3 << 20)):
        c = Composer(0x5E0600 + i)
        while len(c.out) < total:
            n = c.rng.randint(16384, 131072)
            r = c.rng.random() if i != 1 else 1.0
            if r < 0.1:
                c.stored(c.rng.randbytes(c.rng.randint(1, 65535)))
            elif r < 0.2:
                c.static(n)
            elif r < 0.27:
                c.dynamic(n, hlit_pad=c.rng.randint(1, 20), hdist_pad=c.rng.randint(1, 3))
            elif r < 0.3:
                c.dynamic(0, lit_code="eob-only")
            else:
                c.dynamic(n, lit_shape=c.rng.choice(LIT_SHAPES),
                          off_shape=c.rng.choice(LIT_SHAPES), d_use=list(range(30)))
        c.static(10, final=1)
        c.tags.add("multi-block")
        cs.append(_case(f"multi{total >> 20}M", c))
    # what only the reference accepts, in blocks of a stream long enough for
    # the single-buffer path: aliased symbols, HLIT 288 / HDIST 32, one-bit
    # distance codes read from '1', an empty offset code used by matches
    c = Composer(0x5E0680)
    c.dynamic(40000, d_use=list(range(30)))
    for k in range(24):
        r = k % 4
        if r == 0:
            c.dynamic(c.rng.randint(8000, 40000), len_use=list(range(257, 288)),
                      d_use=list(range(32)), lit_shape=LIT_SHAPES[k % 5])
        elif r == 1:
            c.dynamic(c.rng.randint(8000, 40000), hlit_pad=31, hdist_pad=31)
        elif r == 2:
            c.dynamic(c.rng.randint(2000, 9000), off_code="single",
                      d_use=[c.rng.randrange(12)])
        else:
            c.dynamic(c.rng.randint(2000, 9000), off_code="empty")
    c.static(10, final=1)
    cs.append(_case("multi-ref-only", c))
    return cs


def _invalid_cases():
    """each damage after a valid block"""
    cs = []

    def dyn_bad(name, **kw):
        c = Composer(0x5E0700 + len(cs))
        c.static(200)
        c.dynamic(3000, final=1, **kw)
        c.tags.add(name)
        cs.append(_case(name, c, valid=False))

    def over(which):
        def m(stage, obj):
            if stage == "lens":
                ll, dl = obj
                code = ll if which == "lit" else dl
                code[code.index(0)] = max(code)
            elif stage == "pre" and which == "pre":
                z = [s for s in (18, 0, 17, 16) if obj[s] == 0][0]
                obj[z] = max(obj)
        return m

    def under(which):
        def m(stage, obj):
            if stage == "lens" and which != "pre":
                ll, dl = obj
                code = ll if which == "lit" else dl
                i = max(range(len(code)), key=lambda s: (code[s], s != 256))
                code[i] = 0
            elif stage == "pre" and which == "pre":
                i = max(range(19), key=lambda s: obj[s])
                obj[i] = 0
        return m

    for which in ("lit", "off", "pre"):
        dyn_bad(f"bad:oversub-{which}", mutate=over(which), d_use=list(range(12)))
        dyn_bad(f"bad:incomplete-{which}", mutate=under(which), d_use=list(range(12)))

    def len2(stage, obj):
        if stage == "lens":
            obj[1][:] = [0] * 32
            obj[1][0] = 2
    dyn_bad("bad:single-cw-len2", mutate=len2)

    def pre16(stage, obj):
        if stage == "items":
            obj.insert(0, (16, 3))
    dyn_bad("bad:pre16-first", mutate=pre16)

    def overshoot(stage, obj):
        if stage == "items":
            obj[-1] = (18, 138)
    dyn_bad("bad:pre-overshoot", mutate=overshoot)
    dyn_bad("bad:no-eob", lit_code="no-eob")

    c = Composer(0x5E0780)
    c.static(300)
    c.stored(b"abc" * 10, final=1, nlen_xor=0x0100)
    cs.append(_case("bad:stored-nlen", c, valid=False))
    c = Composer(0x5E0781)
    c.dynamic(5000)
    c.static(100, final=1, bad_dist=True)
    cs.append(_case("bad:dist-beyond", c, valid=False))
    c = Composer(0x5E0782)
    c.static(500)
    c.w.put(1, 1)
    c.w.put(3, 2)
    c.w.put(0x5A5A, 16)
    c.tags.add("bad:btype3")
    cs.append(_case("bad:btype3", c, valid=False))
    # truncations of valid streams at each of the last 12 bytes; an output
    # space one byte short
    base = []
    for k, seed in enumerate((0x5E0790, 0x5E0791)):
        c = Composer(seed)
        c.dynamic(4000, lit_shape="tail")
        c.static(300, final=1)
        base.append(_case(f"trunc-base{k}", c))
    for k in range(1, 13):
        b = base[k % 2]
        cs.append(Case(f"bad:trunc{k}", "deflate", b.data[:-k], None, {f"bad:trunc{k}"},
                       avail=len(b.out)))
    for b in base:
        cs.append(Case(f"bad:short-1({b.name})", "deflate", b.data, None, {"bad:short-1"},
                       avail=len(b.out) - 1))
    return cs


def _wrapped(cases):
    """zlib and gzip versions of the small valid raw cases, and a few
    invalid ones"""
    out = []
    for i, cs in enumerate(cases):
        if len(cs.data) > 70000 or i % 2 or cs.name.startswith("tb:"):
            continue        # (the tb: cases end in padding)
        if cs.valid:
            out.append(Case(cs.name + "/zlib", "zlib", zlib_wrap(cs.data, cs.out), cs.out,
                            cs.tags | {"zlib"}, cs.ref_only, ordinary=cs.ordinary))
            out.append(Case(cs.name + "/gzip", "gzip", gzip_wrap(cs.data, cs.out), cs.out,
                            cs.tags | {"gzip"}, cs.ref_only, ordinary=cs.ordinary))
        else:
            out.append(Case(cs.name + "/gzip", "gzip", gzip_wrap(cs.data, b""), None,
                            cs.tags | {"gzip"}, avail=cs.avail))
    return out


def gzip_members(cases, seed=0x5E0900):
    """multi-member gzip concatenations of the valid raw cases (fmt "gzip",
    out: every member's output one after the other)"""
    rng = random.Random(seed)
    small = [c for c in cases if c.valid and c.fmt == "deflate" and len(c.data) < 70000
             and not c.name.startswith("tb:")]
    res = []
    for k in (2, 5, 17):
        pick = rng.sample(small, k)
        res.append(Case(f"members{k}", "gzip",
                        b"".join(gzip_wrap(c.data, c.out) for c in pick),
                        b"".join(c.out for c in pick), {"gzip-members"},
                        any(c.ref_only for c in pick)))
    return res


def dict_cases():
    """raw and zlib streams whose distances reach into a preset dictionary,
    up to its first usable byte; a distance one further, a wrong footer and
    a wrong DICTID as invalid cases"""
    cs = []
    rng = random.Random(0x5E0A00)
    for i, n in enumerate((1, 1000, 32768, 40000)):
        d = rng.randbytes(n)
        c = Composer(0x5E0A10 + i, d)
        c.dynamic(3000, d_use=list(range(30)))
        c.static(4000, final=1)
        raw = c.finish()
        for fmt in ("deflate", "zlib"):
            data = raw if fmt == "deflate" else zlib_wrap(raw, c.out, d)
            cs.append(Case(f"dict{n}/{fmt}", fmt, data, c.out,
                           c.tags | {"dict-raw" if fmt == "deflate" else "dict-zlib"},
                           c.ref_only, dictionary=d))
        if n < 32768:       # (no distance reaches past a full window)
            c = Composer(0x5E0A20 + i, d)
            c.static(0, final=1, bad_dist=True)
            cs.append(Case(f"bad:dict-beyond{n}", "deflate", c.finish(), None, c.tags,
                           avail=700, dictionary=d))
        if i == 1:
            good = cs[-2]
            bad = bytearray(good.data)
            bad[-1] ^= 1
            cs.append(Case("bad:footer", "zlib", bytes(bad), None, {"bad:footer"},
                           avail=len(good.out), dictionary=d))
            bad = bytearray(good.data)
            bad[3] ^= 4
            cs.append(Case("bad:dictid", "zlib", bytes(bad), None, {"bad:dictid"},
                           avail=len(good.out), dictionary=d))
    return cs


def corpus():
    """every case without a dictionary, small ones first"""
    raw = _ref_only_cases() + _plain_cases() + _invalid_cases() + _long_cases()
    return raw + _wrapped(raw)


def tally(cases, extra=()):
    seen = {}
    for c in list(cases) + list(extra):
        for t in c.tags:
            seen[t] = seen.get(t, 0) + 1
    return seen
