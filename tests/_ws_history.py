"""Workspace histories: what a composite call may find in the engine's workspace when it starts.

Every composite entry point runs in ONE grow-only byte buffer (HipEngine.workspace, cffm_amd/engine.py) that comes from
torch.empty and whose layout the library recomputes from B on every call (cffm_ws_layout, cffm_amd/csrc/api.hip): the bytes of
one member at one batch size are another member's at the next.  Nothing clears it, so "every slab, partial and word that is read
has been written by this sequence" is a contract of the kernels, and the results of a sequence must not depend, bit for bit, on
what the buffer held on entry.  This module builds the member map of a layout and the histories that dirty a buffer
(tests/test_ws_history_cpu.py checks the map on the host, tests/test_gpu_ws_history.py runs the sequences).

No tests in here.  The map and the integer fills are numpy only; the functions that touch an engine import torch lazily.
"""
import numpy as np

FLOAT, INT, SIZE = 'float', 'int', 'size'

# Every field of cffm_ws_layout_t (include/cffm_hip.h), by name: the kind of what lies at that offset, or SIZE for a field that
# is no offset (a byte / float / partial count).  A field that is not listed is an error in member_map(), never a default: a new
# member has to be classified before the histories may write over it.
MEMBER_KINDS = {
    'bytes': SIZE,
    'Ei': FLOAT, 'Eo': FLOAT, 'fb': FLOAT, 'inner_out': FLOAT, 'C': FLOAT,
    't1': FLOAT, 'h1': FLOAT, 'att': FLOAT, 'out': FLOAT, 'sqerr': FLOAT, 'scalars': FLOAT, 'dout': FLOAT, 'dt1': FLOAT,
    'dC': FLOAT, 'dEi': FLOAT, 'dEo': FLOAT, 'dfb': FLOAT,
    'gpart': FLOAT, 'gpart_floats': SIZE,
    'sort_keys': INT, 'sort_vals': INT,          # 64-bit keys (id << 32 | slot), unsorted and sorted (api.hip, cffm_ws_layout_from)
    'sort_tmp': INT, 'sort_tmp_bytes': SIZE,     # scratch of the radix sort and of the scans
    'Gi': FLOAT, 'Go': FLOAT, 'Gfb': FLOAT,
    'pool': FLOAT, 'pool_np': SIZE,
    'w0pack': FLOAT, 'w0pack_floats': SIZE,
    'relu0': INT,                                # one bit per element of C[0] .. C[live-2]
    'wb3': FLOAT, 'wb3_bytes': SIZE,             # bf16 pieces: counted as float (0xFF.. is a NaN and 0x7F7F a finite 3.39e38 there too)
}

# Members that carry state from one sequence to the next BY DESIGN and are therefore left out of a history, each with the file and
# line that says so.  There is none: every member is rebuilt by the sequence that reads it.  (The dense image `flat` of
# cffm_dp_local_dense is zero on entry by contract - include/cffm_hip.h, "CONTRACT of the image" - but it is a buffer of its own, not
# a member of the workspace.)  tests/test_ws_history_cpu.py pins this list.
EXEMPT = {}

HISTORIES = ('zeros', 'leftover', 'nan', 'huge')
NAN_WORD = -1                   # 0xFFFFFFFF: a NaN as fp32 and, in both halves, as bf16
HUGE_WORD = 0x7F7F7F7F          # 3.39e38 as fp32 (finite), 3.39e38 as bf16


def member_map(wl, kinds=None):
    """[(name, byte offset, byte length, kind)] of the used members of one cffm_ws_layout_t, in offset order.  An array field gives
    one entry per used element ('C[0]', 'pool[2]').  A member at offset 0 is "not used" (the struct is zeroed first and only the
    members of this shape are laid out) - except gpart, which IS the first member (api.hip: "first: offset 0").  The length of a
    member is the distance to the next used offset, or to `bytes`: the alignment padding behind a member belongs to it."""
    kinds = MEMBER_KINDS if kinds is None else kinds
    if int(wl.gpart) != 0 or int(wl.gpart_floats) <= 0:
        raise ValueError('the member map expects gpart to be the first, non-empty member of the workspace')
    found = []
    for field in type(wl)._fields_:
        name = field[0]
        if name not in kinds:
            raise ValueError('cffm_ws_layout_t field %r is not classified in tests/_ws_history.py MEMBER_KINDS' % name)
        if kinds[name] == SIZE:
            continue
        v = getattr(wl, name)
        offs = [('%s[%d]' % (name, i), int(o)) for i, o in enumerate(v)] if hasattr(v, '__len__') else [(name, int(v))]
        for n, off in offs:
            if off == 0 and name != 'gpart':
                continue
            found.append((off, n, kinds[name]))
    found.sort(key=lambda e: e[0])
    ends = [e[0] for e in found[1:]] + [int(wl.bytes)]
    return [(n, off, end - off, kind) for (off, n, kind), end in zip(found, ends)]


def overlaps(map_a, map_b):
    """[(member of b, member of a)] for every float member of layout b that shares bytes with a DIFFERENT member of layout a: what a
    run at batch a leaves where a run at batch b keeps that member."""
    out = []
    for nb, ob, lb, kb in map_b:
        if kb != FLOAT or lb == 0:
            continue
        for na, oa, la, _ in map_a:
            if na != nb and la > 0 and oa < ob + lb and ob < oa + la:
                out.append((nb, na))
    return out


def int_fill(name, nbytes, M, n_slots, rng):
    """Valid but wrong content for the integer member `name` of nbytes bytes, as a uint8 array (None: leave the member as it is).
    Integer members never get wild values: a kernel that wrongly consumes a stale index must show as a bit mismatch, never as an
    access out of range.
      sort_keys   64-bit keys id << 32 | slot with ids drawn from [0, M) and the slots a random permutation of [0, n_slots)
      sort_vals   the same kind of keys, sorted: a well-formed run of other ids
      relu0       random bits
      sort_tmp    None: it keeps the bytes the leftover run in front of the fill left there"""
    if name == 'sort_tmp':
        return None
    if name in ('sort_keys', 'sort_vals'):
        n = nbytes // 8
        ids = rng.integers(0, M, size=n).astype(np.int64)
        slots = np.resize(rng.permutation(n_slots), n).astype(np.int64)
        keys = (ids << 32) | slots
        if name == 'sort_vals':
            keys = np.sort(keys)
        out = np.zeros(nbytes, dtype=np.uint8)
        out[:n * 8] = keys.view(np.uint8)
        return out
    if name == 'relu0':
        return rng.integers(0, 256, size=nbytes).astype(np.uint8)
    raise ValueError('no integer fill for workspace member %r' % name)


def theta_ranges(tl):
    """[(name, first float, end)] of the members of theta in offset order (the ranges the slab plan is made of)."""
    offs = [(int(getattr(tl, m)), m) for m in ('att_W', 'att_b', 'bias', 'inner_cw', 'inner_cb', 'inner_dw', 'inner_db', 'd1_w', 'd1_b',
                                                'd2_w', 'd2_b', 'lin_w', 'lin_b')]
    for l in range(int(tl.live)):
        offs += [(int(tl.conv_w[l]), 'conv_w[%d]' % l), (int(tl.conv_b[l]), 'conv_b[%d]' % l)]
    offs.sort()
    ends = [o for o, _ in offs[1:]] + [int(tl.n)]
    return [(m, o, e) for (o, m), e in zip(offs, ends)]


def theta_range_of(tl, index):
    for m, o, e in theta_ranges(tl):
        if o <= index < e:
            return '%s + %d' % (m, index - o)
    return 'past theta.n (+%d)' % (index - int(tl.n))


# ---- the histories, on an engine ------------------------------------------------------------------------------------------------
def pool_buffer(eng, *batches):
    """The engine's ONE workspace buffer, grown to what every batch size of `batches` asks for."""
    for B in batches:
        eng.workspace(B)
    return eng._pool.buf


def zeros(eng, B):
    pool_buffer(eng, B).zero_()


def fill(eng, B, word, seed=0):
    """The WHOLE buffer (not only layout(B).bytes): float members of the layout of B and everything behind the layout get `word`,
    integer members their int_fill()."""
    import torch
    buf = pool_buffer(eng, B)
    _, wl = eng.workspace(B)
    assert buf.numel() % 4 == 0 and buf.data_ptr() % 4 == 0
    words = buf.view(torch.int32)
    rng = np.random.default_rng(seed)
    for name, off, ln, kind in member_map(wl):
        if name.split('[')[0] in EXEMPT or ln == 0:
            continue
        if kind == FLOAT:
            words[off // 4:(off + ln) // 4].fill_(word)
            continue
        data = int_fill(name, ln, int(eng.cfg.M), int(B) * int(eng.cfg.F), rng)
        if data is not None:
            buf[off:off + ln].copy_(torch.from_numpy(data))
    words[int(wl.bytes) // 4:].fill_(word)


def leftover(eng, params, B, B_other, run):
    """`run(eng)` - a real call at batch B_other with other ids - leaves its bytes in the buffer; the parameters, the optimizer slots
    and the step counter are then put back with load_params.  The buffer must not move across that: the case that follows has to
    run on those very bytes."""
    buf = pool_buffer(eng, B, B_other)
    ptr = buf.data_ptr()
    acc, acc2 = eng.export_accumulators(), eng.export_second_moments()
    run(eng)
    eng.load_params(params, accs=acc, accs2=acc2)
    eng.opt_step = 0
    assert eng._pool.buf.data_ptr() == ptr, 'the workspace buffer moved across the leftover run'


def enter(history, eng, params, B, B_other, run, seed=0):
    """Dirty `eng`'s workspace with one of HISTORIES in front of a sequence at batch B.  nan and huge sit on top of a leftover run
    (sort_tmp then holds genuine bytes of that run)."""
    if history == 'zeros':
        return zeros(eng, B)
    leftover(eng, params, B, B_other, run)
    if history == 'nan':
        fill(eng, B, NAN_WORD, seed)
    elif history == 'huge':
        fill(eng, B, HUGE_WORD, seed)
    elif history != 'leftover':
        raise ValueError(history)


def first_mismatch(got, ref):
    """Flat index of the first element where assert_array_equal's notion of equality fails (NaN == NaN), or None."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return 0
    bad = ~((got == ref) | ((got != got) & (ref != ref)))
    return int(np.flatnonzero(bad.reshape(-1))[0]) if bad.any() else None


def assert_same(history, name, got, ref, tl=None):
    """np.testing.assert_array_equal(got, ref) with a message that names the history, the tensor and the first differing index -
    and, for a tensor laid out like theta (tl given), the theta range that index falls in."""
    got, ref = np.asarray(got), np.asarray(ref)
    try:
        np.testing.assert_array_equal(got, ref)
    except AssertionError:
        i = first_mismatch(got, ref)
        where = '' if tl is None or i is None else ' (theta range %s)' % theta_range_of(tl, i)
        n_bad = int((~((got == ref) | ((got != got) & (ref != ref)))).sum()) if got.shape == ref.shape else -1
        raise AssertionError('history %s: %s differs from the zeros run, first at flat index %s%s: %r against %r; %d of %d elements differ'
                             % (history, name, i, where, got.reshape(-1)[i] if i is not None else None,
                                ref.reshape(-1)[i] if i is not None else None, n_bad, got.size))


# ---- the cases: which (shape, B) a sequence is entered at, and which batch size the leftover run in front of it has --------------
# train-step cases, Adagrad: names of tests/test_gpu_parity.py CASES (the smallest shapes that reach each route), no heavy one
TRAIN_CASES = ('frappe-selu', 'f10-d32-b100-elu', 'f7-d32-b64-gelu', 'f7-d32-b63-gelu', 'f11-d32-b256-relu', 'f6-d64-b256-elu',
               'b257-relu', 'b1-elu', 'f16-d32-b130', 'f16-k32-d32-b70-selu', 'f20-k32-d32-b3-relu', 'f33-d32-relu', 'f20-d64-elu',
               'f10-k20-d16-elu', 'd128-f3-k12-gelu', 'no-inner', 'no-outer', 'fm-only-nolinatt', 'frappe-b1024-dups')
# (B of the leftover run, B of the case) at the frappe shape: across the slab-plan changes at 64, 256, 257..1023 and 1024
PAIR_SHAPE = dict(M=900, F=10, K=32, D=32, act='selu')
FRAPPE_PAIRS = ((300, 100), (100, 300), (1024, 64), (64, 65), (256, 257))
OPT_CASES = ('f10-d32-b100-elu', 'f16-d32-b130')
OPTIMIZERS = ('GradientDescentOptimizer', 'MomentumOptimizer', 'AdamOptimizer')
LOSS_SHAPE = dict(M=80, F=4, K=8, D=8, act='elu', B=12)           # the 'tmp-' shape of test_gpu_parity.test_other_losses
LOSSES = ('square_l2', 'mae', 'log_loss', 'hybrid')
SEQUENCE_CASES = ('frappe-selu', 'f10-d32-b100-elu', 'f16-k32-d32-b70-selu')
PACKED_CASES = ('f20-k64-b7-gelu', 'f28-k32-b10-elu')             # the two packed cases of tests/test_gpu_branches.py
EVAL_BATCHES = (1, 63, 64, 65, 100, 256, 257, 300, 1023, 1024)    # the batch sizes the CPU test lays every shape out at


def pair_name(B_other, B):
    return 'pair-b%d-after-b%d' % (B, B_other)


def pair_case(B):
    return dict(PAIR_SHAPE, B=B)


def leftover_batch(B):
    """Batch size of the leftover run in front of a case at batch B that is not one of FRAPPE_PAIRS: 2 B + 1 - every member behind
    gpart moves, and most land inside another member - except above 300, where a smaller batch (another slab regime) does the same
    for less."""
    return 2 * B + 1 if B <= 300 else 300
