"""Plain-Python restatement of the chemical fingerprint and the graph key ("Chemical fingerprints"),
written from nothing but that definition: what `tests/test_fingerprint_host.py` and `tests/test_fingerprint_gpu.py` hold
the HIP kernel to.  A molecule is (z, adj, n): atomic numbers, a symmetric n x n list of bond codes 0 none / 1 / 2 / 3 /
4 aromatic, and the atom count.  Pass Python ints."""
M = 0xFFFFFFFF
SEED = 0x6d636731
W2 = {1: 2, 2: 4, 3: 6, 4: 3}          # twice the bond order, aromatic = 1.5


def rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M


def mm3(words, seed):
    """MurmurHash3_x86_32 of the little-endian bytes of a sequence of uint32 words."""
    h = seed & M
    for k in words:
        k = (k & M) * 0xcc9e2d51 & M
        k = rotl(k, 15)
        k = k * 0x1b873593 & M
        h ^= k
        h = rotl(h, 13)
        h = (h * 5 + 0xe6546b64) & M
    h ^= 4 * len(words)
    h ^= h >> 16
    h = h * 0x85ebca6b & M
    h ^= h >> 13
    h = h * 0xc2b2ae35 & M
    h ^= h >> 16
    return h


def ring_sizes(n, adj):
    """ring(a): the size of the smallest cycle through atom a, 0 if it lies on none."""
    nbrs = [[j for j in range(n) if j != a and adj[a][j]] for a in range(n)]
    out = []
    for a in range(n):
        best = 0
        for j in nbrs[a]:                 # the shortest way from a to j that does not use the bond a-j:
            dist = {a: 0}                 # breadth first from a's other neighbours, a itself closed
            frontier = [k for k in nbrs[a] if k != j]
            for k in frontier:
                dist[k] = 1
            d = 1
            while frontier and j not in dist:
                d += 1
                nxt = []
                for u in frontier:
                    for v in nbrs[u]:
                        if v not in dist:
                            dist[v] = d
                            nxt.append(v)
                    if j in dist:         # its level is final; the rest of this level cannot change it
                        break
                frontier = nxt
            if j in dist:
                size = dist[j] + 1
                best = size if best == 0 else min(best, size)
        out.append(best)
    return out


def layers(z, adj, n, rounds):
    """The invariants inv_0 .. inv_rounds, one list per round."""
    ring = ring_sizes(n, adj)
    nbrs = [[j for j in range(n) if j != a and adj[a][j]] for a in range(n)]
    inv = [mm3([0, z[a], len(nbrs[a]), sum(W2[adj[a][j]] for j in nbrs[a]), ring[a]], SEED) for a in range(n)]
    yield inv
    for r in range(1, rounds + 1):
        new = []
        for a in range(n):
            words = [r, inv[a]]
            for c, i in sorted((adj[a][j], inv[j]) for j in nbrs[a]):
                words += [c, i]
            new.append(mm3(words, SEED))
        inv = new
        yield inv


def fingerprint(z, adj, n, radius=2, nbits=2048):
    """The set of set bits."""
    bits = set()
    for inv in layers(z, adj, n, radius):
        for v in inv:
            bits.add(v & (nbits - 1))
    return bits


def key(z, adj, n):
    inv = None
    for inv in layers(z, adj, n, max(n - 1, 2)):       # K = max(n - 1, 2) rounds
        pass
    s = sorted(inv) if inv else []
    return (mm3([n] + s, SEED ^ 0x9e3779b9) << 32) | mm3([n] + s, SEED)


def fingerprint_and_key(z, adj, n):
    """(`fingerprint`, `key`) from one pass over the rounds."""
    bits, inv = set(), None
    for r, inv in enumerate(layers(z, adj, n, max(n - 1, 2))):
        if r <= 2:
            bits.update(v & 2047 for v in inv)
    s = sorted(inv) if inv else []
    return bits, (mm3([n] + s, SEED ^ 0x9e3779b9) << 32) | mm3([n] + s, SEED)


def mol(zs, bonds):
    """(z, adj, n) from atomic numbers and (i, j, code) bonds."""
    n = len(zs)
    adj = [[0] * n for _ in range(n)]
    for i, j, c in bonds:
        adj[i][j] = adj[j][i] = c
    return list(zs), adj, n


def permute(z, adj, n, p):
    """The same molecule with new atom i = old atom p[i]."""
    return [z[p[i]] for i in range(n)], [[adj[p[i]][p[j]] for j in range(n)] for i in range(n)], n


def words(bits):
    """A bit set as the 64 uint32 words of the stored fingerprint."""
    out = [0] * 64
    for k in bits:
        out[k >> 5] |= 1 << (k & 31)
    return out


def tanimoto(a, b):
    """fp32 Tanimoto of two bit sets: NaN where either is empty (a molecule without atoms)."""
    import numpy as np
    if not a or not b:
        return np.float32("nan")
    return np.float32(len(a & b)) / np.float32(len(a | b))
