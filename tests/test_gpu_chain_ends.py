"""The two ends of the chained layer-1 launch (locator_amd/csrc/l1_chain.hip, round 8): its prologue stages the first TWO
super-tiles of every workgroup (row indices read by the loader lanes themselves, dZ, both sets of small operands and the first
unit requested back to back, one drain), and its last step runs on dummy requests.  What a workgroup owns decides which of
those are real: with one super-tile per workgroup the prologue's second fetch is a dummy, with `n_super - 1` workgroups exactly
one workgroup owns two, with one workgroup everything runs through the loop.  So `loc_l1_backward_adam_chain` is called
directly (the harness of tests/test_gpu_chain.py::test_chain_kernel_against_the_two_kernels_it_replaces) for every such
`grid`, on NaN-filled partial buffers between guard margins:

1. W1, gamma, beta, b1, all their Adam moments and the next step's [scale|shift|mean|rstd] are BIT-IDENTICAL for every grid:
   none of them depends on how the k-tiles are dealt out (the forward partials do: they are compared as a float64 sum);
2. they match loc_l1_backward_adam + loc_l1_forward within that test's bars;
3. the product library and the drained twin (every hand-counted wait = vmcnt(0)) agree bit for bit, each in its own process;
4. nothing outside the first grid * KTW partial groups is written (and nothing at all without a next minibatch);
5. a two-row-block fit (batch 64, width 256) equals the unchained schedule;
6. the hidden-layer / head Adam tail as trailing workgroups of the launch equals the tail as a launch of its own, bit for bit
   (the last step of an epoch has no next minibatch: rows_next = NULL with a tail)."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import bits, build_net, guarded, make_problem, maxerr, poison

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256, 512)
# 3 k-tiles (less than one super-tile at width 64, a short second one at width 128); 32 k-tiles; 125 k-tiles (a short last
# super-tile at widths 64 and 128)
KS = (96, 1000, 4000)
ROWS = ((1, 1), (17, 5), (32, 32))
N = 80


def grids_of(n_super):
    """One workgroup; one super-tile per workgroup; one workgroup with two; three or so each."""
    out = []
    for g in (1, n_super, n_super - 1, -(-n_super // 3)):
        if g >= 1 and g not in out:
            out.append(g)
    return out


def _launch_chain(net, rows, n_b, rows_next, n_b_next, next_stats, bn4, dz, grid, partial):
    from locator_amd import _lib
    lib, d, lay = net.lib, net.d, net.lay
    Pp, Mp, Vp = net.params.data_ptr(), net.adam_m.data_ptr(), net.adam_v.data_ptr()
    o = lambda base, off: C.c_void_p(base + 4 * off)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.loc_l1_backward_adam_chain(
        C.c_void_p(net.X.data_ptr()), net.X.stride(0), C.c_void_p(rows.data_ptr()), n_b,
        C.c_void_p(rows_next.data_ptr()) if rows_next is not None else None, n_b_next, C.byref(d), C.c_void_p(bn4.data_ptr()),
        C.c_void_p(next_stats.data_ptr()) if rows_next is not None else None, C.c_void_p(dz.data_ptr()),
        o(Pp, lay.w1), o(Mp, lay.w1), o(Vp, lay.w1), o(Pp, lay.gamma), o(Pp, lay.beta), o(Mp, lay.gamma), o(Vp, lay.gamma),
        o(Mp, lay.beta), o(Vp, lay.beta), o(Pp, lay.b1), o(Mp, lay.b1), o(Vp, lay.b1),
        C.c_void_p(net.alpha_tab.data_ptr()), len(net.alpha_tab), C.c_void_p(net.lr_t.data_ptr()),
        C.c_void_p(net.t_base_t.data_ptr()), 1, grid, C.c_void_p(partial.data_ptr()), partial.numel(),
        C.byref(net.tuning), st), "chain")


def _launch_pair(net, rows, n_b, rows_next, n_b_next, next_stats, bn4, dz):
    """The two kernels the chained one replaces -> the next minibatch's layer-1 activations."""
    from locator_amd import _lib
    lib, d, lay = net.lib, net.d, net.lay
    Kp, Hp = d.Kp, d.Hp
    Pp, Mp, Vp = net.params.data_ptr(), net.adam_m.data_ptr(), net.adam_v.data_ptr()
    o = lambda base, off: C.c_void_p(base + 4 * off)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gbs = torch.zeros(4 * Kp, device="cuda")
    partial = torch.zeros(512 * 32 * Hp, device="cuda")
    a1 = torch.zeros((32, Hp), device="cuda")
    _lib.check(lib.loc_l1_backward_adam(
        C.c_void_p(net.X.data_ptr()), net.X.stride(0), C.c_void_p(rows.data_ptr()), n_b, C.byref(d),
        C.c_void_p(bn4.data_ptr()), C.c_void_p(dz.data_ptr()),
        o(Pp, lay.w1), o(Mp, lay.w1), o(Vp, lay.w1), o(Pp, lay.gamma), o(Pp, lay.beta), o(Mp, lay.gamma), o(Vp, lay.gamma),
        o(Mp, lay.beta), o(Vp, lay.beta), o(Pp, lay.b1), o(Mp, lay.b1), o(Vp, lay.b1), C.c_void_p(gbs.data_ptr()),
        C.c_void_p(net.alpha_tab.data_ptr()), len(net.alpha_tab), C.c_void_p(net.lr_t.data_ptr()),
        C.c_void_p(net.t_base_t.data_ptr()), 1, net.l1_bwd_grid, C.c_void_p(next_stats.data_ptr()),
        C.c_void_p(bn4.data_ptr()), None, C.byref(net.tuning), st), "backward")
    _lib.check(lib.loc_l1_forward(
        C.c_void_p(net.X.data_ptr()), net.X.stride(0), C.c_void_p(rows_next.data_ptr()), n_b_next, C.byref(d),
        C.c_void_p(bn4.data_ptr()), o(Pp, lay.w1), o(Pp, lay.b1), C.c_void_p(partial.data_ptr()), net.l1_fwd_grid,
        C.c_void_p(a1.data_ptr()), None, None, C.c_float(1.0), st), "forward")
    return a1


@functools.lru_cache(maxsize=None)
def case_digest(width, K):
    """Every (n_b, n_b_next) x grid of one (width, K): assertions 1, 2 and 4 of the module docstring -> sha256 over what the
    chained launches left (parameters, moments and bn4 once per row case - they are the same for every grid - and every grid's
    partial groups), for the comparison of the two libraries."""
    h = hashlib.sha256()
    x, y, p, rng = make_problem(N, K, width, 2, seed=1000 * width + K)
    net = build_net(x, y, p, drop_p=0.0)
    d, lay = net.d, net.lay
    Kp, Hp = d.Kp, d.Hp
    assert Hp == width
    ktw = max(1, 8 // (Hp // 32))
    assert ktw == int(net.lib.loc_l1_chain_groups_per_workgroup(Hp))
    n_super = -(-(Kp // 32) // ktw)
    dev = "cuda"
    # non-trivial Adam state and a third step, second moments of the size of the squared first moments (as in a real fit)
    net.adam_m.copy_(torch.from_numpy(rng.normal(0, 1e-3, net.adam_m.numel()).astype(np.float32)))
    net.adam_v.copy_(torch.from_numpy(((0.5 + rng.random(net.adam_v.numel())) * 1e-6).astype(np.float32)))
    pad = torch.arange(Kp, device=dev) >= K                       # padded SNPs carry zero state, as after init / import
    for buf in (net.adam_m, net.adam_v):
        buf[lay.gamma:lay.gamma + Kp][pad] = 0
        buf[lay.beta:lay.beta + Kp][pad] = 0
    net.t_base_t.fill_(2)
    P0, M0, V0 = net.params.clone(), net.adam_m.clone(), net.adam_v.clone()
    sl = lambda off, n: slice(off, off + n)
    sections = (("W1", lay.w1, Hp * Kp), ("gamma", lay.gamma, Kp), ("beta", lay.beta, Kp), ("b1", lay.b1, Hp))

    def restore():
        net.params.copy_(P0); net.adam_m.copy_(M0); net.adam_v.copy_(V0)

    for n_b, n_b_next in ROWS:
        rows = torch.from_numpy(rng.choice(N, 32, replace=False).astype(np.int32)).to(dev)
        rows_next = torch.from_numpy(rng.choice(N, 32, replace=False).astype(np.int32)).to(dev)
        dz = torch.zeros((32, Hp), device=dev)
        dz[:n_b] = torch.from_numpy(rng.normal(0, 0.05, (n_b, Hp)).astype(np.float32)).to(dev)   # rows beyond n_b are zero

        def stats_of(r, n):       # [mean | biased var] of a minibatch, [2][Kp]
            xb = x[r.cpu().numpy()[:n]].astype(np.float64)
            s = np.zeros((2, Kp), np.float32)
            s[0, :K], s[1, :K] = xb.mean(0), xb.var(0)
            return torch.from_numpy(s).to(dev)

        next_stats = stats_of(rows_next, n_b_next).contiguous()
        cur = stats_of(rows, n_b)
        g, b = P0[lay.gamma:lay.gamma + Kp], P0[lay.beta:lay.beta + Kp]
        rstd = torch.where(pad, torch.zeros_like(cur[1]), 1.0 / torch.sqrt(cur[1] + 1e-3))
        bn4_in = torch.cat([g * rstd, b - cur[0] * (g * rstd), cur[0], rstd]).contiguous()

        # the two kernels it replaces
        restore()
        bn4 = bn4_in.clone()
        a1_ref = _launch_pair(net, rows, n_b, rows_next, n_b_next, next_stats, bn4, dz)
        torch.cuda.synchronize()
        ref = dict(P=net.params.cpu().numpy(), M=net.adam_m.cpu().numpy(), V=net.adam_v.cpu().numpy(),
                   bn4=bn4.cpu().numpy(), a1=a1_ref.cpu().numpy())
        assert np.abs(ref["P"][sl(lay.w1, Hp * Kp)] - P0.cpu().numpy()[sl(lay.w1, Hp * Kp)]).max() > 1e-4     # it did train

        first = None
        for grid in grids_of(n_super) + [None]:                  # None: no next minibatch (grid: one super-tile each)
            chain = grid is not None
            g_eff = grid if chain else n_super
            n_body = g_eff * ktw * 32 * Hp
            partial, check = guarded(n_body)
            poison(partial, "nan")
            restore()
            bn4 = bn4_in.clone()
            _launch_chain(net, rows, n_b, rows_next if chain else None, n_b_next if chain else 0, next_stats, bn4, dz,
                          g_eff, partial)
            what = f"width {width} K {K} rows {n_b}/{n_b_next} grid {grid}"
            check(what)                                          # 4. nothing outside the grid * KTW groups ...
            got = (bits(net.params), bits(net.adam_m), bits(net.adam_v))
            if not chain:
                assert bool((bits(partial) == -1).all()), what   # ... and nothing at all without a next minibatch
                assert torch.equal(bits(bn4), bits(bn4_in)), what
                for a, b_ in zip(got, first[:3]):
                    assert torch.equal(a, b_), what              # the backward half does not depend on the forward half
                continue
            assert not bool(torch.isnan(partial).any()), what    # every group of the launch was written
            if first is None:
                first = got + (bits(bn4),)
                for t in first:
                    h.update(t.numpy().tobytes())
                # 2. against the two kernels (bars of test_chain_kernel_against_the_two_kernels_it_replaces)
                Pn, Mn, Vn = (t.numpy().view(np.float32) for t in got)
                for name, off, n in sections:
                    assert maxerr(ref["P"][sl(off, n)], Pn[sl(off, n)]) < 2e-6, (what, name)
                    assert maxerr(ref["M"][sl(off, n)], Mn[sl(off, n)]) < 1e-6, (what, name)
                    np.testing.assert_allclose(Vn[sl(off, n)], ref["V"][sl(off, n)], rtol=2e-3, atol=1e-13, err_msg=name)
                np.testing.assert_allclose(bn4.cpu().numpy(), ref["bn4"], rtol=2e-6, atol=2e-6)
            else:                                                # 1. bit-identical for every grid
                for name, a, b_ in zip(("params", "adam_m", "adam_v", "bn4"), got + (bits(bn4),), first):
                    assert torch.equal(a, b_), (what, name, int((a != b_).sum()))
            h.update(bits(partial).numpy().tobytes())
            z = partial.view(g_eff * ktw, 32, Hp).double().sum(0) + net.params[lay.b1:lay.b1 + Hp].double()
            a1 = torch.where(z > 0, z, torch.expm1(z)).cpu().numpy()
            assert maxerr(ref["a1"][:n_b_next], a1[:n_b_next]) < 2e-5 * max(1.0, float(np.abs(ref["a1"]).max())), what
    return h.hexdigest()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("width", WIDTHS)
def test_chain_launch_is_the_same_for_every_grid_and_matches_the_two_kernels(width, K):
    case_digest(width, K)


_DIGESTS = """
import sys
sys.path.insert(0, sys.argv[2])
from locator_amd import _lib
_lib.use_library(sys.argv[1])
from tests.test_gpu_chain_ends import KS, WIDTHS, case_digest
for w in WIDTHS:
    for K in KS:
        print("DIGEST", w, K, case_digest(w, K))
"""


def test_chain_ends_equal_the_drained_build_bit_for_bit(tmp_path):
    """3. Every case above again in a process of its own on liblocator_hip_drain.so (all of its assertions included); what the
    launches left must carry the digests of the product library."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    drain = os.path.join(root, "locator_amd", "liblocator_hip_drain.so")
    assert os.path.exists(drain), "locator_amd/liblocator_hip_drain.so not built (make -C locator_amd/csrc debug_drain)"
    script = tmp_path / "chain_ends_digests.py"
    script.write_text(_DIGESTS)
    r = subprocess.run([sys.executable, str(script), drain, root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    theirs = {tuple(l.split()[1:3]): l.split()[3] for l in r.stdout.splitlines() if l.startswith("DIGEST")}
    ours = {(str(w), str(K)): case_digest(w, K) for w in WIDTHS for K in KS}
    assert theirs == ours


def test_two_row_block_chain_equals_the_unchained_schedule():
    """5. l1_bwd_adam_chain_kernel<13, 8, 2> (batch 64 at width 256: 32 dZ words per thread in the prologue, eleven loader
    roles): minibatches of 64 and 36 rows (the last step uses both blocks, 4 rows of the second), three epochs."""
    from tests.test_gpu_chain import _assert_same_fit, _run_epochs
    x, y, p, rng = make_problem(120, 3000, 256, 4, seed=64)
    tr, va = np.arange(100), np.arange(100, 120)
    perms = [np.random.default_rng(80 + e).permutation(100) for e in range(3)]
    _, h0, p0, m0, v0, _ = _run_epochs(x, y, p, tr, va, perms, False, 0.25, True, batch=64)
    _, h1, p1, m1, v1, _ = _run_epochs(x, y, p, tr, va, perms, True, 0.25, True, batch=64)
    assert maxerr(h0, h1) < 2e-5, (h0, h1)
    _assert_same_fit(p0, p1, m0, m1, v0, v1)
    assert np.abs(p1["W"][0] - p["W"][0]).max() > 1e-4


@pytest.mark.parametrize("width", WIDTHS)
def test_tail_inside_the_chained_launch_equals_the_tail_as_its_own_launch(width):
    """6. Two chained epochs of 32, 32, 6 rows with the hidden-layer / head Adam tail as trailing workgroups of the layer-1
    launch (default) and as loc_stack_dw_adam's own launch (tuning chain_tail = -1): losses, every weight and every Adam
    moment bit for bit.  The last step of an epoch runs without a next minibatch."""
    from locator_amd.train import EpochRunner
    x, y, p, rng = make_problem(90, 2100, width, 4, seed=width + 6)
    out = []
    for tuning in (None, {"chain_tail": -1}):
        net = build_net(x, y, p, drop_p=0.25, seed=5, tuning=tuning)
        r = EpochRunner(net, np.arange(70), np.arange(70, 90), 32, use_graph=False, chain=True)
        assert r.chain and net.tuning.chain_tail == (0 if tuning is None else -1)
        hist = [r.run_epoch(np.random.default_rng(3 + e).permutation(70)) for e in range(2)]
        torch.cuda.synchronize()
        out.append((np.float64(hist).tobytes(), bits(net.params), bits(net.adam_m), bits(net.adam_v)))
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert torch.equal(a, b), int((a != b).sum())
