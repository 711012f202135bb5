"""Block auditor for DEFLATE streams (pure Python, no GPU).

walk() decodes a raw DEFLATE / zlib / gzip stream and returns, for every
block, what the compressor decided: its type and bit range, the code lengths
and header fields of a dynamic block, the precode items, the histograms of
the symbols actually decoded and the (length, distance) pairs with the
symbols and extra bits used for them.

Next to it are plain, exact references of what the compressor is meant to
compute (RFC 1951 and the documented method of deflate_huffman.h /
deflate_kernel.hip, restated from their comments):

  huffman_cost         optimal unlimited-length cost (heapq)
  package_merge        optimal length-limited cost
  restated_make_code   make_code(): rank sort on (freq, sym), two-queue merge
                       with the leaf winning a tie, leaves per depth, clamp
                       with the zlib-style Kraft repair, longest codewords to
                       the rarest symbols, {s, s ? 0 : 1} when m < 2
  precode_items_ref    greedy run-length coding of the code lengths
  static_cost / stored_cost / dynamic_cost
                       the block-end cost model

and audit_stream(), which checks every block against them.  Every check has
a name (CHECKS); a violation is reported as (check, block index, message).
"""
import heapq
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51,
            59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4,
             4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257,
             385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9,
              10, 10, 11, 11, 12, 12, 13, 13]
PERM = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
PRE_EXTRA = {16: 2, 17: 3, 18: 7}
STATIC_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
STATIC_D = [5] * 32

CHECKS = ("code_limits", "kraft", "used_iff_coded", "optimal", "restated_lens",
          "header_trim", "precode_items", "cost_exact", "choice", "stored_shape",
          "symbols")


class StreamError(ValueError):
    pass


def ll_extra(sym):
    return LEN_EXTRA[sym - 257] if 257 <= sym <= 285 else 0


def d_extra(sym):
    return DIST_EXTRA[sym] if sym < 30 else 0


def len_sym(length):
    """the canonical litlen symbol of a match length (258 -> 285)"""
    if length == 258:
        return 285
    for i in range(27, -1, -1):
        if LEN_BASE[i] <= length:
            return 257 + i
    raise ValueError(length)


def dist_sym(dist):
    for i in range(29, -1, -1):
        if DIST_BASE[i] <= dist:
            return i
    raise ValueError(dist)


# ---------------------------------------------------------------- walker

def _rev(v, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def canonical_codes(lens):
    """canonical codewords (MSB-first); codewords that do not fit their
    length (an oversubscribed code) are None"""
    bl = [0] * 64
    for ln in lens:
        bl[ln] += 1
    bl[0] = 0
    nxt, code = [0] * 64, 0
    for b in range(1, 64):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for ln in lens:
        if ln == 0:
            out.append(None)
            continue
        c = nxt[ln]
        nxt[ln] += 1
        out.append(c if c < (1 << ln) else None)
    return out


def _table(lens):
    """LSB-first decode table: (1 << maxbits) entries of sym << 4 | len"""
    mb = max(lens) if lens else 0
    if mb == 0:
        return [], 0
    tbl = [None] * (1 << mb)
    for sym, (ln, c) in enumerate(zip(lens, canonical_codes(lens))):
        if c is None:
            continue
        r = _rev(c, ln)
        e = (sym << 4) | ln
        for k in range(0, 1 << mb, 1 << ln):
            if tbl[r | k] is None:
                tbl[r | k] = e
    return tbl, mb


def strip_container(data, fmt):
    """-> raw DEFLATE bytes (the trailer is left on: the walker stops at the
    final block)"""
    data = bytes(data)
    if fmt == "deflate":
        return data
    if fmt == "zlib":
        if len(data) < 6 or (data[0] * 256 + data[1]) % 31 or data[0] & 15 != 8:
            raise StreamError("bad zlib header")
        return data[6:] if data[1] & 0x20 else data[2:]
    if fmt == "gzip":
        if len(data) < 18 or data[:3] != b"\x1f\x8b\x08":
            raise StreamError("bad gzip header")
        flg, p = data[3], 10
        if flg & 4:
            p += 2 + data[p] + 256 * data[p + 1]
        for bit in (8, 16):
            if flg & bit:
                p = data.index(b"\0", p) + 1
        if flg & 2:
            p += 2
        return data[p:]
    raise ValueError(fmt)


class Block:
    """One block as walk() saw it.  Bits are counted from the start of the
    raw DEFLATE data; out_start from the end of the dictionary."""

    def __init__(self, btype, final, start_bit, out_start):
        self.type, self.final = btype, final
        self.start_bit, self.end_bit = start_bit, None
        self.out_start, self.out_len = out_start, 0
        self.hlit = self.hdist = self.hclen = None
        self.ll_lens = self.d_lens = self.pre_lens = None
        self.pre_items = None               # [(sym, repeat count or None)]
        self.ll_hist = [0] * 288
        self.d_hist = [0] * 32
        self.pre_hist = [0] * 19
        self.matches = []                   # [(length, dist, lsym, lextra, dsym, dextra)]
        self.stored_len = self.stored_nlen = self.pad_bits = None

    @property
    def bits(self):
        return self.end_bit - self.start_bit

    def __repr__(self):
        return ("Block(type=%d final=%d bits=[%d,%d) out=[%d,+%d))" %
                (self.type, self.final, self.start_bit, self.end_bit,
                 self.out_start, self.out_len))


def walk(data, fmt="deflate", dictionary=b""):
    """-> (decoded bytes, [Block]).  Raises StreamError on what no decoder
    accepts (a codeword that is not in its code, a distance too far back)."""
    raw = strip_container(data, fmt)
    d = raw + bytes(8)
    nbits = 8 * len(raw)
    out = bytearray(dictionary)
    base = len(dictionary)
    blocks = []
    pos = 0

    def get(n):
        nonlocal pos
        if pos + n > nbits:
            raise StreamError("stream ends inside a block")
        p = pos >> 3
        v = (int.from_bytes(d[p:p + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def decoder(lens):
        tbl, mb = _table(lens)
        mask = (1 << mb) - 1

        def dec():
            nonlocal pos
            p = pos >> 3
            e = tbl[(int.from_bytes(d[p:p + 3], "little") >> (pos & 7)) & mask] \
                if mb else None
            if e is None:
                raise StreamError("codeword not in the code")
            pos += e & 15
            if pos > nbits:
                raise StreamError("stream ends inside a codeword")
            return e >> 4
        return dec

    while True:
        b = Block(None, None, pos, len(out) - base)
        b.final = get(1)
        b.type = get(2)
        if b.type == 3:
            raise StreamError("block type 3")
        if b.type == 0:
            pad = (-pos) & 7
            b.pad_bits = get(pad) if pad else 0
            b.stored_len, b.stored_nlen = get(16), get(16)
            p = pos >> 3
            if pos + 8 * b.stored_len > nbits:
                raise StreamError("stored block past the end")
            out += raw[p:p + b.stored_len]
            pos += 8 * b.stored_len
        else:
            if b.type == 2:
                b.hlit, b.hdist, b.hclen = 257 + get(5), 1 + get(5), 4 + get(4)
                b.pre_lens = [0] * 19
                for i in range(b.hclen):
                    b.pre_lens[PERM[i]] = get(3)
                pdec = decoder(b.pre_lens)
                lens, items = [], []
                while len(lens) < b.hlit + b.hdist:
                    s = pdec()
                    b.pre_hist[s] += 1
                    if s < 16:
                        items.append((s, None))
                        lens.append(s)
                        continue
                    if s == 16:
                        if not lens:
                            raise StreamError("repeat of no length")
                        r = 3 + get(2)
                        lens += [lens[-1]] * r
                    else:
                        r = (3 + get(3)) if s == 17 else (11 + get(7))
                        lens += [0] * r
                    items.append((s, r))
                if len(lens) != b.hlit + b.hdist:
                    raise StreamError("code lengths overrun HLIT + HDIST")
                b.pre_items = items
                b.ll_lens = lens[:b.hlit] + [0] * (288 - b.hlit)
                b.d_lens = lens[b.hlit:] + [0] * (32 - b.hdist)
                if b.ll_lens[256] == 0:
                    raise StreamError("no end-of-block codeword")
                lens_ll, lens_d = b.ll_lens, b.d_lens
            else:
                lens_ll, lens_d = STATIC_LL, STATIC_D
            ldec, ddec = decoder(lens_ll), decoder(lens_d)
            llh, dh, ms = b.ll_hist, b.d_hist, b.matches
            while True:
                s = ldec()
                llh[s] += 1
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise StreamError("litlen symbol %d" % s)
                ne = LEN_EXTRA[s - 257]
                le = get(ne) if ne else 0
                length = LEN_BASE[s - 257] + le
                ds = ddec()
                if ds >= 30:
                    raise StreamError("distance symbol %d" % ds)
                dh[ds] += 1
                de = get(DIST_EXTRA[ds]) if DIST_EXTRA[ds] else 0
                dist = DIST_BASE[ds] + de
                if dist > len(out):
                    raise StreamError("distance %d too far back" % dist)
                ms.append((length, dist, s, le, ds, de))
                if dist >= length:
                    out += out[len(out) - dist:len(out) - dist + length]
                else:
                    for _ in range(length):
                        out.append(out[-dist])
        b.end_bit = pos
        b.out_len = len(out) - base - b.out_start
        blocks.append(b)
        if b.final:
            break
    return bytes(out[base:]), blocks


# ---------------------------------------------------------------- references

def code_cost(freq, lens):
    return sum(f * ln for f, ln in zip(freq, lens))


def huffman_cost(freq):
    """optimal (unlimited length) cost sum f * len; one used symbol costs a
    1-bit codeword"""
    w = [f for f in freq if f]
    if len(w) < 2:
        return sum(w)
    heapq.heapify(w)
    cost = 0
    while len(w) > 1:
        s = heapq.heappop(w) + heapq.heappop(w)
        cost += s
        heapq.heappush(w, s)
    return cost


def package_merge(freq, limit):
    """optimal cost of a code whose lengths are <= limit (Larmore-Hirschberg):
    the 2m - 2 cheapest items of the last merged list"""
    leaves = sorted(f for f in freq if f)
    m = len(leaves)
    if m < 2:
        return sum(leaves)
    if m > (1 << limit):
        raise ValueError("no code of %d symbols fits %d bits" % (m, limit))
    items = list(leaves)
    for _ in range(limit - 1):
        pk = [items[i] + items[i + 1] for i in range(0, len(items) - 1, 2)]
        items = list(heapq.merge(leaves, pk))
    return sum(items[:2 * m - 2])


def restated_make_code(freq, maxlen, info=None):
    """make_code() of deflate_huffman.h as its comments describe it -> lens.
    info (a dict) receives m, the unclamped depth and whether it clamped."""
    n = len(freq)
    lens = [0] * n
    order = sorted((f, s) for s, f in enumerate(freq) if f)
    m = len(order)
    if info is not None:
        info.update(m=m, depth=1, clamped=False)
    if m < 2:
        s = order[0][1] if m else 0
        lens[s] = 1
        lens[0 if s else 1] = 1
        return lens
    A = [f for f, _ in order]
    NW, P = [0] * (m - 1), [0] * (m - 1)
    leaf = node = 0
    for k in range(m - 1):
        w = 0
        for _ in range(2):
            if leaf < m and (node == k or A[leaf] <= NW[node]):
                w += A[leaf]
                leaf += 1
            else:
                w += NW[node]
                P[node] = k
                node += 1
        NW[k] = w
    root = m - 2
    depth = [0] * (m - 1)
    for k in range(root - 1, -1, -1):
        depth[k] = depth[P[k]] + 1
    maxd = max(depth) + 1
    cntI = [0] * (maxd + 2)
    for dd in depth:
        cntI[dd] += 1
    cnt = [0] * (max(maxd, maxlen) + 2)
    for dd in range(1, maxd + 1):
        cnt[dd] = 2 * cntI[dd - 1] - cntI[dd]
    if info is not None:
        info.update(depth=maxd, clamped=maxd > maxlen)
    over = sum(cnt[maxlen + 1:])
    if over:
        cnt[maxlen] += over
        for dd in range(maxlen + 1, len(cnt)):
            cnt[dd] = 0
        kraft = sum(cnt[dd] << (maxlen - dd) for dd in range(1, maxlen + 1))
        while kraft > (1 << maxlen):
            dd = maxlen - 1
            while cnt[dd] == 0:
                dd -= 1
            cnt[dd] -= 1
            cnt[dd + 1] += 2
            cnt[maxlen] -= 1
            kraft -= 1
    i = 0
    for dd in range(maxlen, 0, -1):
        for _ in range(cnt[dd]):
            lens[order[i][1]] = dd
            i += 1
    return lens


def precode_items_ref(lens):
    """run-length items of the concatenated code lengths, greedy as
    lib/deflate_compress.c:1482-1557 does it -> [(sym, repeat count or None)]"""
    items, i, n = [], 0, len(lens)
    while i < n:
        v, j = lens[i], i
        while j < n and lens[j] == v:
            j += 1
        left = j - i
        if v == 0:
            while left >= 11:
                r = min(left, 138)
                items.append((18, r))
                left -= r
            if left >= 3:
                items.append((17, left))
                left = 0
        elif left >= 4:
            items.append((v, None))
            left -= 1
            while left >= 3:
                r = min(left, 6)
                items.append((16, r))
                left -= r
        items += [(v, None)] * left
        i = j
    return items


def trimmed_counts(ll_lens, d_lens):
    """HLIT, HDIST as the kernel trims them"""
    hlit = max([257] + [s + 1 for s in range(257, 288) if ll_lens[s]])
    hdist = max([1] + [s + 1 for s in range(32) if d_lens[s]])
    return hlit, hdist


def trimmed_hclen(pre_lens):
    n = 19
    while n > 4 and pre_lens[PERM[n - 1]] == 0:
        n -= 1
    return n


def token_bits(ll_hist, d_hist, ll_lens, d_lens):
    bits = 0
    for s, f in enumerate(ll_hist):
        if f:
            bits += f * (ll_lens[s] + ll_extra(s))
    for s, f in enumerate(d_hist):
        if f:
            bits += f * (d_lens[s] + d_extra(s))
    return bits


def static_cost(ll_hist, d_hist):
    return 3 + token_bits(ll_hist, d_hist, STATIC_LL, STATIC_D)


def stored_cost(start_bit, blen):
    """stored pieces of at most 65535 bytes: the first one pads to a byte"""
    pieces = max(1, (blen + 65534) // 65535)
    pad = (-(start_bit + 3)) & 7
    return 3 + pad + 32 + 8 * blen + (pieces - 1) * 40


def dynamic_header_ref(ll_lens, d_lens):
    """-> (hlit, hdist, items, pre_hist, pre_lens, hclen) as the block end
    derives them from the code lengths"""
    hlit, hdist = trimmed_counts(ll_lens, d_lens)
    items = precode_items_ref(list(ll_lens[:hlit]) + list(d_lens[:hdist]))
    pre_hist = [0] * 19
    for s, _ in items:
        pre_hist[s] += 1
    pre_lens = restated_make_code(pre_hist, 7)
    return hlit, hdist, items, pre_hist, pre_lens, trimmed_hclen(pre_lens)


def items_bits(items, pre_lens):
    return sum(pre_lens[s] + PRE_EXTRA.get(s, 0) for s, _ in items)


def dynamic_cost(ll_hist, d_hist, ll_lens=None, d_lens=None):
    """bits of a dynamic block for these tokens (codes by restated_make_code
    unless given), header derived as the block end derives it"""
    if ll_lens is None:
        ll_lens = restated_make_code(ll_hist, 15)
    if d_lens is None:
        d_lens = restated_make_code(d_hist, 15)
    _, _, items, _, pre_lens, hclen = dynamic_header_ref(ll_lens, d_lens)
    return (3 + 5 + 5 + 4 + 3 * hclen + items_bits(items, pre_lens) +
            token_bits(ll_hist, d_hist, ll_lens, d_lens))


def kraft_sum(lens):
    """sum 2^-len as a fraction of 2^-15 units (== 1 << 15 for a complete code)"""
    return sum(1 << (15 - ln) for ln in lens if ln)


# ---------------------------------------------------------------- audit

def _forced_pair(lens, hist):
    """the documented form of an alphabet with fewer than two used symbols:
    {s, s ? 0 : 1} one bit each"""
    used = [s for s, f in enumerate(hist) if f]
    if len(used) >= 2:
        return None
    s = used[0] if used else 0
    return {s, 0 if s else 1}


def _audit_code(name, lens, hist, maxlen, v, stats):
    """code_limits / kraft / used_iff_coded / optimal / restated_lens for one
    alphabet"""
    if any(ln > maxlen for ln in lens):
        v("code_limits", "%s length > %d" % (name, maxlen))
    pair = _forced_pair(lens, hist)
    coded = {s for s, ln in enumerate(lens) if ln}
    if pair is not None and coded == pair and all(lens[s] == 1 for s in pair):
        pass
    else:
        if kraft_sum(lens) != 1 << 15:
            v("kraft", "%s Kraft sum %d / 32768" % (name, kraft_sum(lens)))
        used = {s for s, f in enumerate(hist) if f}
        if coded != used:
            v("used_iff_coded", "%s coded-but-unused %s, used-but-uncoded %s" %
              (name, sorted(coded - used), sorted(used - coded)))
    info = {}
    want = restated_make_code(hist, maxlen, info)
    cost = code_cost(hist, lens)
    if info["m"] >= 2 and all(lens[s] for s, f in enumerate(hist) if f):
        # where the unlimited tree fits the limit the code is an optimal one;
        # everywhere it costs at least the length-limited optimum
        if not info["clamped"] and cost != huffman_cost(hist):
            v("optimal", "%s cost %d != Huffman %d" % (name, cost, huffman_cost(hist)))
        if cost < package_merge(hist, maxlen) and max(lens) <= maxlen:
            v("optimal", "%s cost %d below package-merge" % (name, cost))
    if list(lens) != want:
        v("restated_lens", "%s lengths differ from restated_make_code at %s" %
          (name, [s for s in range(len(lens)) if lens[s] != want[s]][:8]))
    if stats is not None:
        stats.note(name, info)


class Coverage:
    """counters of the make_code edges a set of audited streams reached"""

    def __init__(self):
        self.c = {}

    def add(self, key, k=1):
        self.c[key] = self.c.get(key, 0) + k

    def note(self, name, info):
        m = info["m"]
        self.add(name + ":m<2" if m < 2 else name + ":m<24" if m < 24 else name + ":m>=24")
        if info["clamped"]:
            self.add(name + ":clamped")
        if name == "litlen" and (2 <= m <= 3 or 22 <= m <= 26):
            self.add("litlen:m=%s" % ("2-3" if m <= 3 else "22-26"))

    def __getitem__(self, k):
        return self.c.get(k, 0)

    def __repr__(self):
        return repr(dict(sorted(self.c.items())))


def audit_blocks(blocks, stats=None, seg_bytes=None):
    """every invariant on every block -> [(check, block index, message)].
    seg_bytes: the segment size of a stream of the segmented single-buffer
    path, whose segments are joined by a non-final block and an empty stored
    block (host_compress.hip); no other stream may hold an empty stored block
    but the whole stream of an empty input."""
    out = []
    if seg_bytes and blocks:
        total = blocks[-1].out_start + blocks[-1].out_len
        joins = [b.out_start for b in blocks if b.type == 0 and b.stored_len == 0 and
                 not b.final]
        if joins != list(range(seg_bytes, total, seg_bytes)):
            out.append(("stored_shape", 0, "segment joins at %s, segments of %d" %
                        (joins[:8], seg_bytes)))
    for i, b in enumerate(blocks):
        def v(check, msg, i=i, b=b):
            assert check in CHECKS, check
            out.append((check, i, "%r: %s" % (b, msg)))
        if stats is not None:
            stats.add("blocks")
            stats.add("type%d" % b.type)
        for (ln, dist, ls, le, ds, de) in b.matches:
            if ls != len_sym(ln) or ds != dist_sym(dist):
                v("symbols", "length %d as %d+%d, distance %d as %d+%d" %
                  (ln, ls, le, dist, ds, de))
                break
        if b.type == 0:
            if b.stored_nlen != b.stored_len ^ 0xFFFF or b.pad_bits:
                v("stored_shape", "LEN %d NLEN %d pad %d" % (b.stored_len, b.stored_nlen,
                                                             b.pad_bits))
            if b.stored_len == 0:
                join = bool(seg_bytes and not b.final and 0 < i < len(blocks) - 1 and
                            b.out_start % seg_bytes == 0)
                alone = b.final and len(blocks) == 1
                if not (join or alone):
                    v("stored_shape", "empty stored block that is no segment join")
                if stats is not None and join:
                    stats.add("join")
            if b.bits != stored_cost(b.start_bit, b.stored_len):
                v("cost_exact", "stored bits %d != %d" % (b.bits, stored_cost(
                    b.start_bit, b.stored_len)))
            continue
        tokens = token_bits(b.ll_hist, b.d_hist, *(
            (b.ll_lens, b.d_lens) if b.type == 2 else (STATIC_LL, STATIC_D)))
        stat = static_cost(b.ll_hist, b.d_hist)
        stored = stored_cost(b.start_bit, b.out_len)
        if b.type == 1:
            if b.bits != stat:
                v("cost_exact", "static bits %d != %d" % (b.bits, stat))
            dyn = dynamic_cost(b.ll_hist, b.d_hist)
            if not (stat < stored and stat <= dyn):
                v("choice", "static %d, stored %d, dynamic %d" % (stat, stored, dyn))
            continue
        # dynamic
        _audit_code("litlen", b.ll_lens, b.ll_hist, 15, v, stats)
        _audit_code("dist", b.d_lens, b.d_hist, 15, v, stats)
        _audit_code("precode", b.pre_lens, b.pre_hist, 7, v, stats)
        if any(b.ll_lens[s] for s in (286, 287)) or any(b.d_lens[s] for s in (30, 31)):
            v("code_limits", "symbols 286, 287, 30 or 31 have a codeword")
        hlit, hdist = trimmed_counts(b.ll_lens, b.d_lens)
        if (b.hlit, b.hdist, b.hclen) != (hlit, hdist, trimmed_hclen(b.pre_lens)):
            v("header_trim", "HLIT %d HDIST %d HCLEN %d, want %d %d %d" % (
                b.hlit, b.hdist, b.hclen, hlit, hdist, trimmed_hclen(b.pre_lens)))
        items = precode_items_ref(b.ll_lens[:b.hlit] + b.d_lens[:b.hdist])
        if b.pre_items != items:
            v("precode_items", "precode items differ from the greedy run-length coding")
        hdr = 17 + 3 * b.hclen + items_bits(b.pre_items, b.pre_lens)
        if b.bits != hdr + tokens:
            v("cost_exact", "dynamic bits %d != %d" % (b.bits, hdr + tokens))
        if not (b.bits < stat and b.bits < stored):
            v("choice", "dynamic %d, static %d, stored %d" % (b.bits, stat, stored))
    return out


def audit_stream(data, fmt="deflate", dictionary=b"", expect=None, stats=None,
                 seg_bytes=None):
    """walk + audit_blocks; the decoded bytes must be `expect` when given.
    -> (blocks, violations)"""
    out, blocks = walk(data, fmt, dictionary)
    if expect is not None and out != expect:
        raise StreamError("the stream does not decode to its input")
    return blocks, audit_blocks(blocks, stats, seg_bytes)


def zlib_control(data, fmt, dictionary=b""):
    """zlib's decode of the same stream (an independent control of walk())"""
    wb = {"deflate": -15, "zlib": 15, "gzip": 31}[fmt]
    do = zlib.decompressobj(wb, zdict=dictionary) if dictionary else zlib.decompressobj(wb)
    return do.decompress(data) + do.flush()
