"""The contract of the device draws (fcn_draw_batch, csrc/draws.h; INTEGRATION.md "Random draws on the device") restated in
numpy, in the operation order the contract states -- NOT a port of the kernel: no histogram, no select, no bitonic network; a
vectorised Philox4x32-10, np.argsort on the composites and the scalar formulas.  The referee of tests/test_draws_referee.py (known
answers, distribution), tests/test_gpu_draws.py and tests/test_emu_draws.py."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32(ctr, key, rounds=10):
    """ctr (..., 4), key (..., 2) of 32-bit words (broadcast against each other) -> (..., 4) uint32."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], shape).copy() for i in range(4)]
    k = [np.broadcast_to(key[..., i], shape).copy() for i in range(2)]
    for _ in range(rounds):
        p0, p1 = M0 * c[0], M1 * c[2]                           # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> S32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, -1).astype(np.uint32)


def _words(seed, step, b, tag, count):
    """The first `count` 32-bit words of stream `tag` of row b at `step`: word i & 3 of block i >> 2."""
    seed, step = int(seed), int(step)
    nblk = (int(count) + 3) // 4
    ctr = np.empty((nblk, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(nblk, dtype=np.uint64)
    ctr[:, 1] = int(b)
    ctr[:, 2] = step & 0xFFFFFFFF
    ctr[:, 3] = ((step >> 32) << 2) | int(tag)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return philox4x32(ctr, key).reshape(-1)[:int(count)]


def choice_row(seed, step, b, n, N):
    """Row b's N indices from n rows; zeros for a row nothing can be drawn from (n <= 0 or n >= 2^31)."""
    n, N = int(n), int(N)
    if n <= 0 or n >= 2 ** 31:
        return np.zeros(N, dtype=np.int32)
    if n < N:
        w = _words(seed, step, b, 1, N).astype(np.uint64)
        return ((w * np.uint64(n)) >> S32).astype(np.int32)
    k = _words(seed, step, b, 0, n).astype(np.uint64)
    comp = (k << S32) | np.arange(n, dtype=np.uint64)
    return np.argsort(comp, kind="stable")[:N].astype(np.int32)      # composites are unique: any sort gives this order


def _u53(hi, lo):
    return float((int(hi) >> 5) * 2 ** 26 + (int(lo) >> 6))


def scalars_row(seed, step, b, flip=True, shift=True):
    """(coin, normal, hshift) of row b."""
    w = _words(seed, step, b, 2, 8)
    scale = 2.0 ** -53
    coin = _u53(w[0], w[1]) * scale if flip else 0.0
    if not shift:
        return coin, 0.0, 0.5
    u1 = (_u53(w[2], w[3]) + 1.0) * scale
    u2 = _u53(w[4], w[5]) * scale
    normal = float(np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))
    return coin, normal, _u53(w[6], w[7]) * scale


def draw(seed, step, counts, N, flip=True, shift=True, sub=None, sub_off=None):
    """What fcn_draw_batch writes for the rows `counts` at `step`: (choice (B,N) int32, coin, normal, hshift (B) float64, status).
    sub / sub_off: the optional composition (a row with sub_off[b + 1] > sub_off[b] draws from that many and maps through sub)."""
    B = len(counts)
    choice = np.zeros((B, N), dtype=np.int32)
    coin, normal, hshift = np.zeros(B), np.zeros(B), np.zeros(B)
    status = 0
    for b in range(B):
        n, seg = int(counts[b]), None
        if sub is not None and int(sub_off[b + 1]) > int(sub_off[b]):
            seg = np.asarray(sub, dtype=np.int32)[int(sub_off[b]):int(sub_off[b + 1])]
            n = len(seg)
        if n <= 0 or n >= 2 ** 31:
            status |= 1
        row = choice_row(seed, step, b, n, N)
        choice[b] = row if seg is None or n <= 0 else seg[row]
        coin[b], normal[b], hshift[b] = scalars_row(seed, step, b, flip, shift)
    return choice, coin, normal, hshift, status
