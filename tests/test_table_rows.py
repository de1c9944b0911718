"""The numpy twin of cffm_init_table_rows (cffm_amd/spec.py table_rows): the specification of the by-global-row draw of the
embedding tables.  CPU only: the cipher against its published known answers, the property the whole feature rests on (a row
is the same row under every sharding), the distribution, and the float32-vs-float64 error of the twin itself, which is the
floor the GPU test (tests/test_gpu_sharded_class.py) measures the kernel against."""
import numpy as np

from cffm_amd.spec import CFFMConfig, philox4x32_10, table_rows, table_words, unit_normals


def twin_fp32_floor(seed, rows, table, width):
    """(fp64 unit normals, max |fp32 twin - fp64 twin|) over the given global rows: the error, in standard deviations of the
    table, that evaluating log / sqrt / sin / cos in float32 instead of float64 costs the twin itself."""
    words = table_words(seed, rows, table, width)
    z64 = unit_normals(words, width, np.float64)
    z32 = unit_normals(words, width, np.float32)
    assert z32.dtype == np.float32
    return z64, float(np.abs(z32.astype(np.float64) - z64).max())


def test_philox4x32_10_known_answers():
    kat = [('00000000 00000000 00000000 00000000', '00000000 00000000', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
           ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff', '408f276d 41c83b0e a20bc7c6 6d5451fd'),
           ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0', 'd16cfe09 94fdcceb 5001e420 24126ea1')]
    words = lambda s: [int(w, 16) for w in s.split()]
    for ctr, key, want in kat:
        got = philox4x32_10(words(ctr), words(key))
        assert [int(v) for v in got] == words(want), (ctr, key)
    # vectorised: the three cases as one call give the same words
    ctr = np.array([words(c) for c, _, _ in kat], dtype=np.uint64).T
    key = np.array([words(k) for _, k, _ in kat], dtype=np.uint64).T
    got = np.stack(philox4x32_10(tuple(ctr), tuple(key)), axis=1)
    assert got.dtype == np.uint32 and got.tolist() == [words(w) for _, _, w in kat]


def test_a_row_is_the_same_row_under_every_sharding():
    rng = np.random.default_rng(3)
    cfg = CFFMConfig(M=4096, F=4, K=34, D=16)                  # K = 34: the last group of four keeps two columns
    whole = table_rows(cfg, 2021, np.arange(4096))
    assert whole['inner_embeddings'].shape == (4096, 34) and whole['outer_embeddings'].shape == (4096, 16)
    for _ in range(20):
        step = int(rng.integers(1, 9))
        row0 = int(rng.integers(0, 64))
        n = int(rng.integers(1, (4096 - row0 - 1) // step + 1))
        rows = row0 + step * np.arange(n)
        part = table_rows(cfg, 2021, rows)
        for k in ('inner_embeddings', 'outer_embeddings', 'feature_bias'):
            assert part[k].shape[0] == n
            np.testing.assert_array_equal(part[k], whole[k][rows], err_msg='%s rows %d::%d' % (k, row0, step))
    # float32 twin: the same property, and rows beyond 2^32 are rows of their own
    a = table_rows(cfg, 7, np.array([5, 2 ** 33 + 5, 2 ** 32 + 5]), dtype=np.float32)['inner_embeddings']
    assert a.dtype == np.float32 and not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], a[2])
    b = table_rows(cfg, 7, np.array([2 ** 33 + 5]), dtype=np.float32)['inner_embeddings']
    np.testing.assert_array_equal(a[1], b[0])
    # another seed (also in the high word of the key), another model; a disabled branch stays zero
    assert not np.array_equal(table_rows(cfg, 7 + 2 ** 32, [5])['inner_embeddings'], table_rows(cfg, 7, [5])['inner_embeddings'])
    off = table_rows(CFFMConfig(M=8, F=4, K=8, D=8, outer_conv=0), 7, np.arange(8))
    assert not off['outer_embeddings'].any() and off['inner_embeddings'].any()


def test_distribution_of_the_inner_table_and_the_fp32_floor():
    """Inner table at seed 2021, rows 0 .. 2^20 - 1, K = 16: 16.8 M unit normals.  Bounds from the sample size alone: the mean of n
    unit normals has standard deviation 1/sqrt(n), their standard deviation 1/sqrt(2n) - five of those each; Box-Muller on a
    24-bit u1 cannot exceed sqrt(2 * 24 * ln 2) = 5.768."""
    cfg = CFFMConfig(M=1 << 20, F=4, K=16, D=4)
    rows = np.arange(1 << 20)
    t = table_rows(cfg, 2021, rows)
    z = t['inner_embeddings'] / 0.1
    n = z.size
    assert n == 16 << 20
    assert abs(z.mean()) < 5 / np.sqrt(n), z.mean()
    assert abs(z.std() - 1.0) < 5 / np.sqrt(2 * n), z.std()
    assert np.abs(z).max() <= 5.768
    assert t['feature_bias'].shape == (1 << 20, 1) and not t['feature_bias'].any()
    zo = t['outer_embeddings'] / 0.01                             # the other table: other numbers, same law
    assert abs(zo.std() - 1.0) < 5 / np.sqrt(2 * zo.size) and not np.array_equal(zo, z[:, :4])
    # the twin's own float32-vs-float64 error: the floor of the GPU test.  |d z| <= r * |d angle| + |d r|: the float32 angle
    # 2 pi u2 is rounded to half an ulp of 2 pi (2.4e-7), r <= 5.77, so a few 1e-6 at the most; and it cannot be zero
    z64, floor = twin_fp32_floor(2021, rows, 0, 16)
    np.testing.assert_allclose(z64 * 0.1, t['inner_embeddings'], rtol=1e-15, atol=0)
    print('fp32 twin against fp64 twin: max %.3e standard deviations' % floor)
    assert 1e-8 < floor < 1e-5, floor


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """cffm_init_table_rows checks its arguments on the host, before anything is launched: those paths run without a GPU (the
    table pointers below are never dereferenced on the host and no call here gets as far as a launch)."""
    import ctypes as C
    import os

    from cffm_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = hip.load()
    base = dict(M=100, F=4, K=8, D=8, act=0, linear_att=1, inner_conv=1, outer_conv=1, loss=0, lamda_att=1.0, beta_outer=1.0, lr=0.05)
    s = hip.Shape(**base)
    tab = hip.Tables(0x10000, 0x20000, 0x30000)
    call = lambda sh, tb, row0, step, n: lib.cffm_init_table_rows(C.byref(sh) if sh is not None else None, C.byref(tb) if tb is not None else None,
                                                                 2021, row0, step, n, None)
    for row0, step, n in ((-1, 1, 10), (0, 0, 10), (0, -3, 10), (0, 1, -1), (0, 1, 101), (2 ** 62, 2 ** 62, 10)):
        assert call(s, tab, row0, step, n) == 10001, (row0, step, n)
    assert call(None, tab, 0, 1, 10) == 10001 and call(s, None, 0, 1, 10) == 10001
    assert call(s, hip.Tables(0, 0x20000, 0x30000), 0, 1, 10) == 10001          # NULL table of an enabled branch
    assert call(s, hip.Tables(0x10000, 0, 0x30000), 0, 1, 10) == 10001
    assert call(s, hip.Tables(0x10004, 0x20000, 0x30000), 0, 1, 10) == 10001     # not 8-byte aligned
    assert call(hip.Shape(**dict(base, K=7)), tab, 0, 1, 10) == 10001            # odd width
    # n_rows == 0: fine, without a launch - also with K = 34 (even is enough here) and a NULL table of a disabled branch
    assert call(s, tab, 5, 8, 0) == 0
    assert call(hip.Shape(**dict(base, K=34)), tab, 5, 8, 0) == 0
    assert call(hip.Shape(**dict(base, outer_conv=0)), hip.Tables(0x10000, 0, 0x30000), 5, 8, 0) == 0
