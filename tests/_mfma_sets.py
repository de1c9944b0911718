"""Operand sets for cffm_probe_mfma_bf16_once (tests/test_gpu_mfma_model.py): designed dots whose result tells one property of the
bf16 MFMA's accumulate, and a random set in the value ranges of the bf16x3 conv loops.

A designed problem holds 16 dots, one per row i: D[i][j] = s_j (sum_k a[i][k] b[k] + c[i]) with the column scales s_j = +-2^e, so
that every dot is also read with the opposite sign and at other exponents (B[k][j] = b[k] s_j, C[i][j] = c[i] s_j, both exact).
Every set is a dict name -> (A_bits [n,16,32] uint16, B_bits [n,32,16] uint16, C [n,16,16] float32)."""
import numpy as np

from oracle import mfma_model as mm

SCALES = np.array([s * 2.0 ** e for e in (0, 1, 7, -7, 20, -20, 40, -40) for s in (1.0, -1.0)])
SIGNS_ONLY = np.array([1.0, -1.0] * 8)


def _pack(dots, b=None, scales=SCALES):
    """dots: list of (a [32], c); b [32] (ones by default) -> problems of 16 dots (the last one padded with zero dots)."""
    b = np.ones(32) if b is None else np.asarray(b, dtype=np.float64)
    n = (len(dots) + 15) // 16
    A = np.zeros((n, 16, 32))
    Cc = np.zeros((n, 16))
    for d, (a, c) in enumerate(dots):
        A[d // 16, d % 16] = a
        Cc[d // 16, d % 16] = c
    B = np.broadcast_to(b[None, :, None] * scales[None, None, :], (n, 32, 16))
    C = Cc[:, :, None] * scales[None, None, :]
    assert np.array_equal(C.astype(np.float32).astype(np.float64), C)
    return mm.bf16_bits(A), mm.bf16_bits(B), C.astype(np.float32)


def layout_set(seed=0):
    """General integer matrices: every model gives the exact integer result, so a mismatch is the probe's own layout."""
    rng = np.random.default_rng(seed)
    n = 8
    A = rng.integers(-8, 9, size=(n, 16, 32)).astype(np.float64)
    B = rng.integers(-8, 9, size=(n, 32, 16)).astype(np.float64)
    C = rng.integers(-1000, 1001, size=(n, 16, 16)).astype(np.float32)
    return mm.bf16_bits(A), mm.bf16_bits(B), C


def rounding_set():
    """C = 1.5 2^e with an even and an odd last significand bit; the products add q / 4 ulp(C), q = +-1 .. +-7, as one product and
    as |q| products of a quarter ulp in different lane groups."""
    dots = []
    for e in (0, 12):
        ulp = 2.0 ** (e - 23)
        for c in (1.5 * 2.0 ** e, 1.5 * 2.0 ** e + ulp):
            for q in (1, 2, 3, 5, 6, 7, -1, -2, -3, -5, -6, -7):
                a = np.zeros(32)
                a[11] = q * ulp / 4
                dots.append((a, c))
                a = np.zeros(32)
                a[[3, 9, 12, 17, 22, 27, 30][:abs(q)]] = np.sign(q) * ulp / 4
                dots.append((a, c))
    return _pack(dots)


def width_set():
    """One large product beside 31 tiny ones, 1 .. 40 bits below it, with C = 0 and C = 12; then tiny products alone under C = 1.5."""
    out = {}
    for name, tiny_a, bk in (('width-8bit', 1.0, 1.0), ('width-16bit', 255.0 / 128, 255.0 / 128)):
        b = np.full(32, bk)
        b[0] = 1.0
        dots = []
        for gap in range(1, 41):
            for c in (0.0, 12.0):
                a = np.full(32, tiny_a * 2.0 ** -gap)
                a[0] = 1.0
                dots.append((a, c))
        out[name] = _pack(dots, b)
    dots = []
    for gap in range(20, 31):
        dots.append((np.full(32, 2.0 ** -gap), 1.5))          # 32 x 2^-gap = 2^(5 - gap): do they survive together?
        a = np.zeros(32)
        a[19] = 2.0 ** -gap
        dots.append((a, 1.5))
    out['width-under-c'] = _pack(dots)
    return out


def cancel_set():
    """L - L + r: two products that cancel exactly (in one lane group, and in the first and the last), a remainder 1 .. 40 bits
    below them, C = 0 and C = r / 8."""
    dots = []
    L = 255.0 / 128
    for gap in range(1, 41):
        r = 2.0 ** -gap
        for c in (0.0, r / 8):
            a = np.zeros(32)
            a[0], a[1], a[2] = L, -L, r
            dots.append((a, c))
            a = np.zeros(32)
            a[0], a[31], a[16] = L, -L, r
            dots.append((a, c))
    return _pack(dots)


def denormal_set():
    """Denormal products (2^-70 x 2^-70), denormal bf16 inputs, a denormal C, and a normal difference that lands in the denormals."""
    dots = []
    b = np.ones(32)
    b[:8] = 2.0 ** -70
    b[8:16] = 2.0 ** 6
    t = 2.0 ** -70
    for cnt in (1, 3, 8):
        for c in (0.0, 3 * 2.0 ** -145, 2.0 ** -120):
            a = np.zeros(32)
            a[:cnt] = t                                          # cnt products of 2^-140
            dots.append((a, c))
    for mant in (1, 0x55, 0x7f):
        a = np.zeros(32)
        a[8] = mant * 2.0 ** -133                                # a denormal bf16 input times 2^6: a normal product
        dots.append((a, 0.0))
        dots.append((a, 2.0 ** -100))
    a = np.zeros(32)
    a[16], a[17] = 1.5 * 2.0 ** -126, -(2.0 ** -126)            # normal products, denormal sum 2^-127
    dots.append((a, 0.0))
    a = np.zeros(32)
    a[16] = -(2.0 ** -126)
    dots.append((a, 1.5 * 2.0 ** -126))                          # the same through C
    return _pack(dots, b, SIGNS_ONLY)


def _piece(x, level):
    """bf16x3 piece `level` (0, 1, 2) of fp32 x as bf16 bits: the round-to-nearest split of split_bf16x3 (conv.hip)."""
    x = np.asarray(x, dtype=np.float32)
    for _ in range(level):
        p = (mm.bf16_rn_bits(x).astype(np.uint32) << np.uint32(16)).view(np.float32)
        x = (x - p).astype(np.float32)
    return mm.bf16_rn_bits(x)


def random_set(n=2048, seed=1):
    """Problems in the ranges the conv loops see: A a piece of relu(N(0,1)) or of N(0,1) activations / gradients, B a piece of
    N(0, 0.05) filters, C an accumulator of the size a K = 512 .. 1984 sum reaches (or zero, the first step)."""
    rng = np.random.default_rng(seed)
    A = np.empty((n, 16, 32), dtype=np.uint16)
    B = np.empty((n, 32, 16), dtype=np.uint16)
    C = np.empty((n, 16, 16), dtype=np.float32)
    for p in range(n):
        la, lb = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)][p % 6]
        x = rng.standard_normal((16, 32))
        if (p // 6) % 2 == 0:
            x = np.maximum(x, 0)
        A[p] = _piece(x, la)
        B[p] = _piece(rng.standard_normal((32, 16)) * 0.05, lb)
        C[p] = (rng.standard_normal((16, 16)) * (0.0, 0.1, 3.0, 30.0)[(p // 12) % 4]).astype(np.float32)
    return A, B, C


def designed_sets():
    out = {'layout': layout_set(), 'rounding': rounding_set(), 'cancel': cancel_set(), 'denormal': denormal_set()}
    out.update(width_set())
    return out


def run_probe(A, B, C):
    """D [n,16,16] float32 from the device."""
    import ctypes as ct

    import torch

    from cffm_amd import hip
    lib = hip.load()
    a = torch.from_numpy(np.ascontiguousarray(A).view(np.int16)).cuda()
    b = torch.from_numpy(np.ascontiguousarray(B).view(np.int16)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(C)).cuda()
    d = torch.full_like(c, float('nan'))
    st = int(torch.cuda.current_stream().cuda_stream)
    hip.check(lib.cffm_probe_mfma_bf16_once(ct.c_void_p(a.data_ptr()), ct.c_void_p(b.data_ptr()), ct.c_void_p(c.data_ptr()),
                                            ct.c_void_p(d.data_ptr()), int(A.shape[0]), ct.c_void_p(st)))
    torch.cuda.synchronize()
    return d.cpu().numpy()
