"""GPU: the three bf16x3 conv kernels (gemm_tile_b3 forward and input gradient with pack_w_b3_kernel, wgrad3_kernel) on the exact
cases of tests/_b3_exact.py: every output must equal the integer reference BIT FOR BIT, whatever the matrix cores round to, because
no partial sum of these cases ever needs rounding (tests/test_b3_exact_cpu.py proves that for every case).  A record read from the
wrong slot, a cross term skipped or added twice changes an integer and fails here, where the statistical tiers of
tests/test_gpu_layers.py see a relative 2^-16 .. 2^-24 on a few elements and pass.  (Seen red once, with a scratch build that zeroed
the a2 b2 term of gemm_tile_b3 on lane group 3: the a2b2 and both six cases failed on C[1] and dC[0], every other case and the fp32
loops passed; that mutation touches every output, so the distribution tier of the per-layer check caught it too, its hard and bias
tiers did not.)

Driven through the stage entry points on a workspace filled by hand (C[0], dC[1], dt1, the relu mask of C[0]; the filter in theta,
biases zero): cffm_conv_fwd(1), cffm_conv_bwd(1) twice (once with the weight-gradient operands, once with an open gate for the input
gradient) and cffm_reduce_slabs.  The same cases run under CFFM_CONV_FP32=1 in a child process (the variable is latched at first
use): the fp32 MFMA loops must return the same bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cffm_amd.spec import CFFMConfig, init_params  # noqa: E402
from oracle import layer_check as lc  # noqa: E402
from tests import _b3_exact as bx  # noqa: E402

CASES, GEOS = bx.CASES, bx.GEOS

pytestmark = pytest.mark.gpu
IDS = ['%s-%s' % (c[0], c[1]) for c in CASES]
_ENG = {}


def _engine(geo, act):
    from cffm_amd.engine import HipEngine
    if (geo, act) not in _ENG:
        _ENG.clear()                       # one workspace at a time
        torch.cuda.empty_cache()
        F, D, _ = GEOS[geo]
        cfg = CFFMConfig(M=64, F=F, K=8, D=D, activation=act, lamda_att=1.3)
        _ENG[(geo, act)] = (cfg, HipEngine(cfg, params=init_params(cfg, seed=0, dtype=np.float32)))
    return _ENG[(geo, act)]


def check_b3(geo, act, want):
    """The three roles of layer 1 run the bf16x3 instances (want = 1) or, under CFFM_CONV_FP32=1, the fp32 ones (want = 0): asked of
    the library, so that a dispatch change cannot empty these cases."""
    from cffm_amd import hip
    cfg, _ = _engine(geo, act)
    ch = hip.conv_choice(hip.make_shape(cfg), GEOS[geo][2], 1)
    got = (ch.fwd.b3, ch.dgrad.b3, ch.wgrad.b3)
    assert got == (want,) * 3, '%s: layer 1 (fwd, dgrad, wgrad) b3 = %s, these cases are there for %d' % (geo, got, want)
    assert (ch.fwd.NT, ch.fwd.RM, ch.dgrad.NT, ch.dgrad.RM, ch.wgrad.NT) == (8, 2, 8, 2, 8)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def _same(what, got, ref, fails):
    g, r = _bits(got), _bits(ref)
    bad = g != r
    if bad.any():
        at = np.unravel_index(int(np.argmax(bad)), bad.shape)
        fails.append('%s: %d / %d elements differ from the integer reference, first at %s: got %r, want %r' % (
            what, int(bad.sum()), bad.size, at, float(np.asarray(got)[at]), float(np.asarray(ref)[at])))


def _mask_words(c0):
    """relu mask words of a [.., Pp] tensor: bit j of word w = channel 16 w + j > 0 (lc.unpack_mask)."""
    bits = (c0.reshape(-1, 16) > 0).to(torch.int32)
    w = (bits << torch.arange(16, device=c0.device, dtype=torch.int32)).sum(-1)
    return torch.where(w >= 32768, w - 65536, w).to(torch.int16)


def run_one(geo, cls, act):
    """One case through the three kernels; returns the list of failures (empty: every tensor is bit-equal)."""
    from cffm_amd import hip
    from tests.test_gpu_layers import relu_words
    g = bx.Geo(*GEOS[geo])
    cfg, eng = _engine(geo, act)
    B, P, Pp, D = g.B, g.P, eng.tl.Pp, cfg.D
    assert (P, Pp) == (g.P, g.Pp) and eng.tl.live >= 3
    buf, wl = eng.workspace(B)
    lib, s, th, st = eng.lib, eng._s, eng.theta.data_ptr(), eng._stream()
    fails = []
    dev = eng.device
    C0 = eng.ws_tensor(B, 'C', (B, g.Sin, g.Sin, Pp), index=0)
    C1 = eng.ws_tensor(B, 'C', (B, g.So, g.So, Pp), index=1)
    dC0 = eng.ws_tensor(B, 'dC', (B, g.Sin, g.Sin, Pp), index=0)
    dC1 = eng.ws_tensor(B, 'dC', (B, g.So, g.So, Pp), index=1)
    dt1 = eng.ws_tensor(B, 'dt1', (B, 2 * D - 2))
    w_off, b_off = int(eng.tl.conv_w[1]), int(eng.tl.conv_b[1])

    def put_filter(W):
        eng.theta[w_off:w_off + 4 * Pp * Pp].copy_(torch.from_numpy(bx.to_theta_w(g, W).reshape(-1)))
        eng.theta[b_off:b_off + Pp].zero_()

    def put_c0(rows_kv):
        C0.copy_(torch.from_numpy(bx.to_c0(g, rows_kv)))
        if wl.relu0 > 0:
            relu_words(eng, cfg, B, 0).copy_(_mask_words(C0).reshape(B, -1))

    def poison(t):
        t[..., :P].fill_(float('nan'))
        t[..., P:].fill_(1.0)

    # ---- forward ----
    case = bx.build(g, cls, 'fwd', act)
    put_filter(case['W'])
    put_c0(bx.dense(g, case['a'], g.KV).astype(np.float32))
    poison(C1)
    if wl.relu0 > 0:
        relu_words(eng, cfg, B, 1).fill_(0x5555)
    hip.check(lib.cffm_conv_fwd(s, th, buf.data_ptr(), B, 1, st))
    torch.cuda.synchronize()
    z = bx.expected(g, case)['z']
    lc.exact_pads_zero('C[1]', C1, P)
    if wl.relu0 > 0:
        lc.exact_mask('relu mask of C[1]', relu_words(eng, cfg, B, 1), C1)
    _same('C[1]', C1[..., :P].reshape(g.rows, P).cpu().numpy(), np.maximum(z, 0.0), fails)

    # ---- weight and bias gradient (the input gradient of this run is gated by the sparse C[0]: only its zeros are checked) ----
    case = bx.build(g, cls, 'wgrad', act)
    put_c0(bx.dense(g, case['a'], g.KV).astype(np.float32))
    dC1.copy_(torch.from_numpy(bx.to_c1(g, bx.dense(g, case['b'], P))))
    dt1.zero_()
    poison(dC0)
    hip.check(lib.cffm_conv_bwd(s, th, buf.data_ptr(), B, 1, st))
    flat = torch.full((int(eng.tl.n),), float('nan'), dtype=torch.float32, device=dev)
    hip.check(lib.cffm_reduce_slabs(s, buf.data_ptr(), B, flat.data_ptr(), st))
    torch.cuda.synchronize()
    ref = bx.expected(g, case)
    gw = flat[w_off:w_off + 4 * Pp * Pp].reshape(4, Pp, Pp)
    _same('grad W[1]', gw[:, :P, :P].reshape(g.KV, P).cpu().numpy(), ref['gW'], fails)
    _same('grad b[1]', flat[b_off:b_off + P].cpu().numpy(), ref['gb'], fails)
    lc.exact_pads_zero('dC[0]', dC0, P)
    lc.exact_gated_zero('dC[0]', dC0, C0)
    if cls in bx.LIMITED_CLASSES and act == 'relu' and geo == 'f16-d32-b512':
        # the same with every row of dC[1] populated (its third piece in every slab and step); the bias gradient of this run is not exact
        case = bx.build(g, cls, 'wgrad', act, full=True)
        put_c0(bx.dense(g, case['a'], g.KV).astype(np.float32))
        dC1.copy_(torch.from_numpy(bx.to_c1(g, bx.dense(g, case['b'], P))))
        hip.check(lib.cffm_conv_bwd(s, th, buf.data_ptr(), B, 1, st))
        flat.fill_(float('nan'))
        hip.check(lib.cffm_reduce_slabs(s, buf.data_ptr(), B, flat.data_ptr(), st))
        torch.cuda.synchronize()
        gw = flat[w_off:w_off + 4 * Pp * Pp].reshape(4, Pp, Pp)
        _same('grad W[1], every row', gw[:, :P, :P].reshape(g.KV, P).cpu().numpy(), bx.expected(g, case)['gW'], fails)

    # ---- input gradient: an open gate (C[0] = 1, one element in eight 0), the pool gradient in dt1 ----
    case = bx.build(g, cls, 'dgrad', act)
    put_filter(case['W'])
    put_c0(case['gate'])
    dC1.copy_(torch.from_numpy(bx.to_c1(g, bx.dense(g, case['a'], P))))
    dt1.zero_()
    dt1[:, D:D + g.Sin].copy_(torch.from_numpy(case['dt1']))
    poison(dC0)
    hip.check(lib.cffm_conv_bwd(s, th, buf.data_ptr(), B, 1, st))
    torch.cuda.synchronize()
    lc.exact_pads_zero('dC[0]', dC0, P)
    lc.exact_gated_zero('dC[0]', dC0, C0)
    _same('dC[0]', bx.from_c0(g, dC0.cpu().numpy()), bx.expected(g, case)['dA'], fails)
    return fails


def run_all(want_b3):
    """Every case in this process -> {case id: failures}."""
    out = {}
    for (geo, cls, act), cid in zip(CASES, IDS):
        check_b3(geo, act, want_b3)
        try:
            out[cid] = run_one(geo, cls, act)
        except AssertionError as e:
            out[cid] = [str(e)]
    return out


@pytest.fixture(scope='module')
def fp32_twin():
    """The same cases on the fp32 MFMA loops: a fresh child process with CFFM_CONV_FP32=1, once for the module."""
    env = dict(os.environ, CFFM_CONV_FP32='1')
    code = ('import json, sys; sys.path.insert(0, %r); from tests.test_gpu_b3_exact import run_all; '
            'print("TWIN " + json.dumps(run_all(0)))' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, 'fp32-loop child failed (%d):\n%s' % (r.returncode, (r.stdout + r.stderr)[-4000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('TWIN ')][-1]
    return json.loads(line[5:])


@pytest.mark.parametrize('geo,cls,act', CASES, ids=IDS)
def test_b3_exact(geo, cls, act):
    check_b3(geo, act, 1)
    fails = run_one(geo, cls, act)
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('cid', IDS)
def test_fp32_loops_exact(cid, fp32_twin):
    assert fp32_twin[cid] == [], '\n'.join(fp32_twin[cid])
