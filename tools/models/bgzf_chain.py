"""CPU model of the BGZF member finder of bgzf_read_kernels.hip (design aid and
test subject, not product code): file bytes -> the member list, by the steps
the kernels take, with the same bounds.

  candidates   every offset that passes htslib's header rule with a size that
               stays inside the file, in file order, at most `cap` of them
               (cap = min(4 max_members + 1024, n / 16 + 1));
  next         per candidate the index of the candidate that starts where it
               ends (binary search), END at the end of the file, NONE otherwise;
  blocks       the candidate list in blocks of BLOCK; jump tables of 2^k hops
               inside the block give every candidate the candidate at which
               its path leaves the block and the hops it takes to get there;
  top walk     from candidate 0 (which must stand at offset 0) block by block:
               the entry of every block on the true chain and the members
               before it; the chain is good when it leaves at END;
  members      per block, rank r of the path from the entry = member base + r;
  serial walk  when there are more candidates than `cap`: from offset 0,
               header by header.

find(data, max_members) -> (ok, count, members[(offset, size)], path); at most
max_members members are listed, `count` is how many the file has, `path` is
"parallel" or "serial".  `force_serial` selects the walk, as LDA_BGZF_SERIAL
does in the library; the result must not depend on it.

  python tools/models/bgzf_chain.py FILE [max_members]
"""
import sys

SIG = b"\x1f\x8b\x08\x04"
MIN_MEMBER = 28
BLOCK = 1024
END, NONE = 0xFFFFFFFF, 0xFFFFFFFE


def header_size(data, p):
    """member size at offset p by the header rule, or 0"""
    n = len(data)
    if n - p < MIN_MEMBER or data[p:p + 4] != SIG:
        return 0
    if data[p + 10:p + 16] != b"\x06\x00BC\x02\x00":
        return 0
    size = (data[p + 16] | data[p + 17] << 8) + 1
    return size if MIN_MEMBER <= size <= n - p else 0


def cand_cap(n, max_members):
    return min(4 * max_members + 1024, n // 16 + 1)


def candidates(data):
    out, p = [], data.find(SIG)
    while p >= 0:
        size = header_size(data, p)
        if size:
            out.append((p, size))
        p = data.find(SIG, p + 1)
    return out


def _next(cands, n):
    pos = [c[0] for c in cands]
    nxt = []
    for i, (p, size) in enumerate(cands):
        end = p + size
        if end == n:
            nxt.append(END)
            continue
        lo, hi = i + 1, len(cands)
        while lo < hi:
            mid = (lo + hi) // 2
            if pos[mid] < end:
                lo = mid + 1
            else:
                hi = mid
        nxt.append(lo if lo < len(cands) and pos[lo] == end else NONE)
    return nxt


def _tables(nxt, b, block):
    """J[k][t]: the candidate 2^k hops after candidate b * block + t, as an
    index inside the block, or None once the path has left it"""
    lo, hi = b * block, min(len(nxt), (b + 1) * block)
    levels = max(1, (block - 1).bit_length())
    J = [[(nxt[i] - lo) if nxt[i] < hi else None for i in range(lo, hi)]]
    for k in range(1, levels):
        prev = J[-1]
        J.append([None if prev[t] is None else prev[prev[t]] for t in range(hi - lo)])
    return J


def _exits(nxt, block):
    ext, hops = [0] * len(nxt), [0] * len(nxt)
    for b in range((len(nxt) + block - 1) // block):
        J = _tables(nxt, b, block)
        for t in range(len(J[0])):
            cur, cnt = t, 0
            for k in range(len(J) - 1, -1, -1):
                if J[k][cur] is not None:
                    cur, cnt = J[k][cur], cnt + (1 << k)
            ext[b * block + t] = nxt[b * block + cur]
            hops[b * block + t] = cnt + 1
    return ext, hops


def parallel(data, max_members, cands, block=BLOCK):
    n, K = len(data), len(cands)
    nxt = _next(cands, n)
    ext, hops = _exits(nxt, block)
    nblocks = (K + block - 1) // block
    entry, base = [NONE] * nblocks, [0] * nblocks
    ok, count = False, 0
    if K and cands[0][0] == 0:
        cur = 0
        for _ in range(nblocks):        # a bound that does not come from the file
            b = cur // block
            entry[b], base[b] = cur, count
            count += hops[cur]
            cur = ext[cur]
            if cur >= K:
                break
        ok = cur == END
    members = [None] * min(count, max_members) if ok else []
    if ok:
        for b in range(nblocks):
            if entry[b] == NONE:
                continue
            J = _tables(nxt, b, block)
            for r in range(hops[entry[b]]):
                cur = entry[b] - b * block
                for k in range(len(J)):
                    if r >> k & 1:
                        cur = J[k][cur]
                if base[b] + r < max_members:
                    members[base[b] + r] = cands[b * block + cur]
    return ok, count, members


def serial(data, max_members):
    n, pos, count, members = len(data), 0, 0, []
    while pos < n:
        size = header_size(data, pos)
        if not size:
            return False, count, []
        if count < max_members:
            members.append((pos, size))
        count += 1
        pos += size
    return True, count, members


def find(data, max_members, force_serial=False, block=BLOCK):
    data = bytes(data)
    if not data:
        return True, 0, [], "empty"
    cands = candidates(data)
    if force_serial or len(cands) > cand_cap(len(data), max_members):
        return serial(data, max_members) + ("serial",)
    return parallel(data, max_members, cands, block) + ("parallel",)


if __name__ == "__main__":
    blob = open(sys.argv[1], "rb").read()
    mm = int(sys.argv[2]) if len(sys.argv) > 2 else len(blob) // 28 + 1
    a, b = find(blob, mm), find(blob, mm, force_serial=True)
    print(f"{a[3]}: ok={a[0]} members={a[1]} candidates={len(candidates(blob))} "
          f"serial agrees: {a[:3] == b[:3]}")
