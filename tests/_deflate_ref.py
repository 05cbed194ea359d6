"""An independent reading of what the device gzip compressor writes, for test_gzip_host.py and test_gpu_gzip.py.

``inflate_member``  a token-level inflater written from RFC 1951: the block type, the dynamic header as sent, the
                    token list and the bits every part took.  It checks itself against ``zlib``.
``model_tokens``    a sequential restatement of the match finder and parse that the header comment of
                    deflate_core.hpp specifies -- no lanes, barriers or atomics: text of one block -> token list.
``huffman_*`` / ``package_merge_cost`` / ``kraft``   what the code properties are measured against.

Nothing here includes or calls the product's code."""
import heapq
import zlib
from fractions import Fraction

import numpy as np

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def len_symbol(length):
    """(symbol 257 .. 285, extra bits, extra value) of a match length 3 .. 258."""
    for i in range(28, -1, -1):
        if length >= LEN_BASE[i]:
            return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]
    raise ValueError(length)


def dist_symbol(dist):
    """(symbol 0 .. 29, extra bits, extra value) of a match distance 1 .. 32768."""
    for i in range(29, -1, -1):
        if dist >= DIST_BASE[i]:
            return i, DIST_EXTRA[i], dist - DIST_BASE[i]
    raise ValueError(dist)


# ---------------------------------------------------------------------------------------------- the inflater
class _Bits:
    """LSB-first bit reader over bytes."""

    def __init__(self, data, at):
        self.data = data + b"\0" * 8
        self.pos = 8 * at

    def peek(self, n):
        at = self.pos >> 3
        return (int.from_bytes(self.data[at:at + 8], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.pos += n
        return v


def _decode_table(lengths):
    """RFC 1951 3.2.2: canonical codes from code lengths -> {(length, code as sent, first bit first)}: symbol, as a
    lookup by the next ``maxlen`` bits of an LSB-first stream."""
    maxlen = max(lengths) if len(lengths) else 0
    if maxlen == 0:
        return None, 0
    count = [0] * (maxlen + 1)
    for l in lengths:
        if l:
            count[l] += 1
    code, nxt = 0, [0] * (maxlen + 1)
    for bits in range(1, maxlen + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    table = [None] * (1 << maxlen)
    for sym, l in enumerate(lengths):
        if not l:
            continue
        c = nxt[l]
        nxt[l] += 1
        assert c < (1 << l), "over-subscribed code"
        rev = int(format(c, "0%db" % l)[::-1], 2)            # Huffman codes are packed most significant bit first
        for hi in range(0, 1 << maxlen, 1 << l):
            table[hi | rev] = (sym, l)
    return table, maxlen


def _symbol(bits, table, maxlen):
    entry = table[bits.peek(maxlen)]
    assert entry is not None, "a bit pattern that is no code"
    bits.pos += entry[1]
    return entry


def inflate_member(member):
    """One BGZF member -> dict: ``btype``, ``bfinal``, ``tokens`` [(pos, literal) | (pos, length, distance)], ``text``,
    ``bits`` {"header", "tokens", "eob"} and, for a dynamic block, ``hlit`` / ``hdist`` / ``hclen`` (symbol counts),
    ``cl_lens`` (19, by symbol), ``cl_syms`` [(symbol, extra value)] as sent, ``ll_lens`` and ``d_lens``."""
    size = len(member)
    assert member[:4] == b"\x1f\x8b\x08\x04" and member[10:12] == b"\x06\x00" and member[12:16] == b"BC\x02\x00"
    bits = _Bits(member, 18)
    out = {"bfinal": bits.take(1), "btype": bits.take(2)}
    text = bytearray()
    tokens = []
    if out["btype"] == 0:
        bits.pos = (bits.pos + 7) // 8 * 8
        n, nn = bits.take(16), bits.take(16)
        assert n ^ nn == 0xffff
        at = bits.pos // 8
        text += member[at:at + n]
        bits.pos += 8 * n
        out["bits"] = {"header": 8 + 32, "tokens": 8 * n, "eob": 0}
    else:
        assert out["btype"] == 2, "the compressor writes stored and dynamic blocks only"
        hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
        cl_lens = [0] * 19
        for i in range(hclen):
            cl_lens[CL_ORDER[i]] = bits.take(3)
        cl_table, cl_max = _decode_table(cl_lens)
        lens, cl_syms = [], []
        while len(lens) < hlit + hdist:
            sym, _ = _symbol(bits, cl_table, cl_max)
            if sym < 16:
                lens.append(sym)
                cl_syms.append((sym, 0))
            elif sym == 16:
                extra = bits.take(2)
                assert lens, "a repeat with nothing before it"
                lens += [lens[-1]] * (3 + extra)
                cl_syms.append((sym, extra))
            else:
                extra = bits.take(3 if sym == 17 else 7)
                lens += [0] * ((3 if sym == 17 else 11) + extra)
                cl_syms.append((sym, extra))
        assert len(lens) == hlit + hdist, "a repeat runs past the last code length"
        ll_lens, d_lens = lens[:hlit], lens[hlit:]
        assert ll_lens[256], "no code for end-of-block"
        out.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl_lens, cl_syms=cl_syms, ll_lens=ll_lens, d_lens=d_lens)
        header_end = bits.pos
        ll_table, ll_max = _decode_table(ll_lens)
        d_table, d_max = _decode_table(d_lens)
        while True:
            sym, _ = _symbol(bits, ll_table, ll_max)
            if sym < 256:
                tokens.append((len(text), sym))
                text.append(sym)
                continue
            if sym == 256:
                eob = ll_lens[256]
                break
            assert sym <= 285
            length = LEN_BASE[sym - 257] + bits.take(LEN_EXTRA[sym - 257])
            assert d_table is not None, "a match in a block without distance codes"
            dsym, _ = _symbol(bits, d_table, d_max)
            assert dsym <= 29
            dist = DIST_BASE[dsym] + bits.take(DIST_EXTRA[dsym])
            assert dist <= len(text), "a distance before the start of the text"
            tokens.append((len(text), length, dist))
            for _ in range(length):
                text.append(text[-dist])
        out["bits"] = {"header": header_end - 8 * 18, "tokens": bits.pos - eob - header_end, "eob": eob}
    # the checks of itself: the text, and the place of the trailer
    assert bytes(text) == zlib.decompress(member, 31)
    assert (bits.pos + 7) // 8 == size - 8, "the block does not end where the trailer starts"
    out["tokens"] = tokens
    out["text"] = bytes(text)
    return out


# ---------------------------------------------------------------------------------------------- the model
TILE = 512                   # positions looked up against one state of the table
SEGMENT = 512                # a match ends at its segment's end
HASH_BITS = 14
WINDOW = 32768


def hash4(keys):
    """The multiplicative hash of 4-byte little-endian keys (a uint32 array)."""
    return ((keys.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(32 - HASH_BITS)


def keys4(arr, n):
    """The 4 bytes at every position 0 .. n - 4 of the uint8 array ``arr`` as uint32."""
    if n < 4:
        return np.zeros((0,), dtype=np.uint32)
    a = arr[:n].astype(np.uint32)
    return a[:n - 3] | (a[1:n - 2] << 8) | (a[2:n - 1] << 16) | (a[3:n] << 24)


def worth(length, dist):
    return length >= 4 + (dist > 256) + (dist > 4096) + (dist > 16384)


def model_matches(text):
    """Per position of the block ``text``: (length, distance) arrays of the match that the finder keeps, 0 for none."""
    n = len(text)
    arr = np.zeros((n + 600,), dtype=np.uint8)
    arr[:n] = np.frombuffer(text, dtype=np.uint8)
    keys = keys4(arr, n)
    hashes = hash4(keys).astype(np.int64)
    best_len = np.zeros((n,), dtype=np.int64)
    best_dist = np.zeros((n,), dtype=np.int64)
    table = np.zeros((1 << HASH_BITS,), dtype=np.int64)              # highest position + 1 by hash
    ks = np.arange(258, dtype=np.int64)
    for lo in range(0, n, TILE):
        hi = min(lo + TILE, n)
        p = np.arange(lo, min(hi, len(keys)), dtype=np.int64)          # a hashed match needs four bytes
        if len(p) and lo:
            cand = table[hashes[p]]
            at = cand - 1
            ok = (cand > 0) & (p - at <= WINDOW)
            ok &= keys[np.maximum(at, 0)] == keys[p]
            p, at = p[ok], at[ok]
            if len(p):
                same = arr[at[:, None] + ks] == arr[p[:, None] + ks]
                length = np.where(same.all(axis=1), 258, same.argmin(axis=1))
                length = np.minimum(length, np.minimum(258, n - p))
                dist = p - at
                keep = length >= 4 + (dist > 256) + (dist > 4096) + (dist > 16384)
                best_len[p[keep]] = length[keep]
                best_dist[p[keep]] = dist[keep]
        q = np.arange(lo, min(hi, len(keys)), dtype=np.int64)          # the tile enters the table after its lookups
        if len(q):
            np.maximum.at(table, hashes[q], q + 1)
    # the distance-1 probe: how far the byte before p repeats from p on
    if n >= 2:
        eq = arr[:n - 1] == arr[1:n]                                   # eq[i]: text[i] == text[i + 1]
        stop = np.flatnonzero(~np.append(eq, False))                   # the first i >= j with eq[i] false ends j's run
        p = np.arange(1, n, dtype=np.int64)
        run = stop[np.searchsorted(stop, p - 1)] - (p - 1)             # common prefix of text[p - 1:] and text[p:]
        run = np.minimum(run, np.minimum(258, n - p))
        win = (run >= 3) & (run >= best_len[p])
        best_len[p[win]] = run[win]
        best_dist[p[win]] = 1
    return best_len, best_dist


def model_tokens(text):
    """The token list of one block: the matches of ``model_matches`` parsed greedily per segment."""
    n = len(text)
    best_len, best_dist = (a.tolist() for a in model_matches(text))
    tokens = []
    for lo in range(0, n, SEGMENT):
        end = min(lo + SEGMENT, n)
        p = lo
        while p < end:
            length = min(best_len[p], end - p)
            if length >= 3:
                tokens.append((p, length, best_dist[p]))
                p += length
            else:
                tokens.append((p, text[p]))
                p += 1
    return tokens


# ---------------------------------------------------------------------------------------------- codes
def kraft(lengths):
    return sum(Fraction(1, 1 << l) for l in lengths if l)


def huffman(freqs):
    """(cost, depth) of an unconstrained Huffman code over the nonzero ``freqs``; among equal weights the shallower
    subtree is merged first, which gives the least depth an optimal code can have."""
    heap = [(int(f), 0) for f in freqs if f]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return cost, heap[0][1]


def package_merge_cost(freqs, maxbits):
    """The least sum of freq * length over prefix codes of at most ``maxbits`` bits (Larmore & Hirschberg)."""
    leaves = sorted(int(f) for f in freqs if f)
    n = len(leaves)
    if n == 1:
        return leaves[0]
    assert n <= (1 << maxbits)
    items = [(w, (i,)) for i, w in enumerate(leaves)]
    level = list(items)
    for _ in range(maxbits - 1):
        pairs = [(level[i][0] + level[i + 1][0], level[i][1] + level[i + 1][1]) for i in range(0, len(level) - 1, 2)]
        level = sorted(items + pairs, key=lambda t: t[0])
    lengths = [0] * n
    for _, members in level[:2 * n - 2]:
        for i in members:
            lengths[i] += 1
    assert kraft(lengths) <= 1
    return sum(w * l for w, l in zip(leaves, lengths))


def token_histograms(tokens):
    """(literal/length frequencies [286] with end-of-block counted once, distance frequencies [30])."""
    ll, d = [0] * 286, [0] * 30
    ll[256] = 1
    for t in tokens:
        if len(t) == 2:
            ll[t[1]] += 1
        else:
            ll[len_symbol(t[1])[0]] += 1
            d[dist_symbol(t[2])[0]] += 1
    return ll, d


def token_bits(tokens, ll_lens, d_lens):
    total = 0
    for t in tokens:
        if len(t) == 2:
            total += ll_lens[t[1]]
        else:
            ls, le, _ = len_symbol(t[1])
            ds, de, _ = dist_symbol(t[2])
            total += ll_lens[ls] + le + d_lens[ds] + de
    return total
