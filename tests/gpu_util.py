"""Helpers shared by the GPU parity tests."""
import numpy as np
import torch

from oracle import locator_oracle as O


def make_problem(n, K, width, nlayers, seed=0, n_na=0):
    rng = np.random.default_rng(seed)
    af = rng.beta(0.4, 0.9, K).clip(0.02, 0.98)
    x = rng.binomial(2, af, (n, K)).astype(np.uint8)
    w = rng.normal(0, 1, (K, 2)) / np.sqrt(K)
    y = (x - x.mean(0)) @ w
    y = (y - y.mean(0)) / y.std(0)
    p = randomize_params(O.init_params(K, width, nlayers, rng), rng, round_fp32=False)
    return x, y, p, rng


def randomize_params(p, rng, round_fp32=True):
    """Make every tensor non-trivial so a dropped term cannot hide.  round_fp32: keep the fp64 oracle's starting
    point exactly representable in fp32, so both sides start from identical values."""
    K = p["gamma"].shape[0]
    p["gamma"] = rng.uniform(0.7, 1.3, K)
    p["beta"] = rng.normal(0, 0.05, K)
    p["mov_mean"] = rng.uniform(0, 1, K)
    p["mov_var"] = rng.uniform(0.2, 1.2, K)
    for l in range(len(p["b"])):
        p["b"][l] = rng.normal(0, 0.05, p["b"][l].shape)
    if round_fp32:
        p = O.cast_params(O.cast_params(p, np.float32), np.float64)
    return p


def build_net(x, y, p, drop_p=0.25, seed=1, **net_kw):
    from locator_amd.net import LocatorNet, upload_genotypes
    K = x.shape[1]
    width = p["W"][0].shape[1]
    nlayers = len(p["W"]) - 2
    X = upload_genotypes(x)
    Y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).cuda()
    net = LocatorNet(X, Y, K, width, nlayers, drop_p, seed=seed, **net_kw)
    net.import_params(O.cast_params(p, np.float32))
    return net


def maxerr(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if np.size(a) else 0.0


def params_err(pa, pb):
    out = {}
    for k in ("gamma", "beta", "mov_mean", "mov_var"):
        if k in pa and k in pb:
            out[k] = maxerr(pa[k], pb[k])
    for l in range(len(pa["W"])):
        out[f"W{l}"] = maxerr(pa["W"][l], pb["W"][l])
        out[f"b{l}"] = maxerr(pa["b"][l], pb["b"][l])
    return out


# ---------------------------------------------------------------- poisoned scratch and guard bands
# (tests/test_gpu_scratch.py, tests/test_gpu_stack_train.py, tests/test_gpu_l1_train.py; the contract is stated in
# include/locator_hip.h, Conventions)
# Scratch comes from torch.empty: in the test processes it is almost always zero or small finite leftovers, in a replicate
# run it holds the previous fit's bytes.  A read of a slot the same call never wrote, or a store one tile past a region, is
# invisible on clean buffers; these helpers make both visible without a sanitizer.

GUARD_BYTES = (0xE1, 0xC3, 0xA5, 0x7F)     # little-endian 0x7FA5C3E1: a NaN with a payload no arithmetic produces


def poison(t, kind, seed=0):
    """Fill the contiguous tensor t in place.  "nan": every 32-bit word 0xFFFFFFFF (every byte 0xFF for uint8) - a NaN as
    fp32, -1 as int32.  "junk": seeded uniform values in +-1e4 (uint8: seeded random bytes) - NaN disappears in fmaxf,
    `x > 0 ? :` and max-reductions, finite junk does not.  "zero": the clean buffer the other two are compared with."""
    assert t.is_contiguous(), "poison() fills contiguous buffers"
    if kind == "zero":
        t.zero_()
    elif kind == "nan":
        if t.dtype == torch.uint8:
            t.fill_(0xFF)
        else:
            assert t.element_size() == 4, t.dtype
            t.view(torch.int32).fill_(-1)
    elif kind == "junk":
        g = torch.Generator(device=t.device)
        g.manual_seed(int(seed))
        if t.dtype == torch.uint8:
            t.random_(0, 256, generator=g)
        else:
            t.uniform_(-1e4, 1e4, generator=g)
    else:
        raise ValueError(f"poison kind {kind!r}")
    return t


def guarded(n, dtype=torch.float32, margin=128 * 256, device="cuda"):
    """-> (view, check): `view` is n elements of `dtype`, 256-byte aligned, inside a larger allocation with at least `margin`
    elements of GUARD_BYTES directly below and directly above it (the view itself starts out as the same pattern);
    check(what) asserts that both margins still hold it.  Use a margin of at least 128 * Hp floats: a 128-row tile is the
    largest unit any kernel stores at once."""
    es = torch.empty(0, dtype=dtype).element_size()
    front = -(-margin * es // 256) * 256
    body = n * es
    total = -(-(front + body + margin * es) // 4) * 4
    raw = torch.tensor(GUARD_BYTES, dtype=torch.uint8, device=device).repeat(total // 4)
    view = raw[front:front + body].view(dtype)
    assert view.numel() == n and view.data_ptr() % 256 == 0, (n, view.data_ptr())
    expect = raw.clone()

    def check(what="buffer"):
        torch.cuda.synchronize()
        for side, lo, hi in (("below", 0, front), ("above", front + body, total)):
            bad = (raw[lo:hi] != expect[lo:hi]).nonzero().flatten()
            assert bad.numel() == 0, (f"{what}: {bad.numel()} bytes of the guard margin {side} the buffer were overwritten "
                                      f"(first at byte {int(bad[0]) + lo - front} relative to the buffer of {body} bytes)")
    return view, check


def scratch_buffers(net, runner=None, with_image=True):
    """The buffers a poisoned run fills: activations, partial sums, statistics, losses and weight images - never rows,
    permutations, offsets or masks.  runner: also its per-step losses / validation distances, the epoch's batch
    statistics (both parities under cross-epoch chaining) and the validation predictions."""
    out = [net.ws]
    if net.ws_predict is not None:
        out.append(net.ws_predict)
    if with_image and net.l1_image is not None:
        out.append(net.l1_image)
    if runner is not None:
        out += [runner.stats, runner.val_yhat] + (list(runner.stats_ep2) if runner.xchain else [runner.stats_ep])
    return out


def poison_scratch(net, runner, kind, seed=0, with_image=True):
    torch.cuda.synchronize()
    for i, t in enumerate(scratch_buffers(net, runner, with_image)):
        poison(t, kind, seed * 16 + i)
    torch.cuda.synchronize()


def swap_scratch(net, runner=None, kind="zero", seed=0):
    """Replace net.ws, net.ws_predict (when present) and net.l1_image by guarded views of EXACTLY the sizes the library asks
    for - loc_workspace_floats_batch for the two workspaces, the largest of loc_l1_image_i8_bytes(d, 3 / 2) and
    loc_l1_image_bytes(d, 3) for the image (none where the width supports no image) - and poison them (and the runner's
    statistics / loss buffers) with `kind`.  Call it after the EpochRunner exists (set_batch may reallocate ws) and before
    its first epoch (the captured graph keeps the pointers).  -> the margins' check callables."""
    import ctypes as C
    lib, d = net.lib, net.d
    margin = 128 * d.Hp
    need = int(lib.loc_workspace_floats_batch(C.byref(d), int(runner.batch) if runner is not None else 32))
    assert need <= net.ws.numel(), (need, net.ws.numel())
    checks = []

    def take(n, dtype, name):
        view, check = guarded(n, dtype, margin * (4 if dtype == torch.uint8 else 1))     # 128 rows of floats either way
        checks.append(lambda: check(name))
        return view
    net.ws = take(need, torch.float32, "ws")
    if net.ws_predict is not None:
        net.ws_predict = take(need, torch.float32, "ws_predict")
    image = max(int(lib.loc_l1_image_i8_bytes(C.byref(d), 3)), int(lib.loc_l1_image_i8_bytes(C.byref(d), 2)),
                int(lib.loc_l1_image_bytes(C.byref(d), 3)))
    net.l1_image = take(image, torch.uint8, "l1_image") if image else None
    net._net = None
    net.params_changed()
    poison_scratch(net, runner, kind, seed)
    return checks


def bits(t):
    """Host copy of a device tensor's raw 32-bit words (NaNs compare by payload, -0.0 differs from 0.0)."""
    return t.detach().contiguous().view(-1).view(torch.int32).cpu()


# ---------------------------------------------------------------- Adam moments against the oracle (tests/test_gpu_moments.py)
# Adam divides the gradient by its own running magnitude, so the weights after Adam hardly see a gradient that is off by
# a constant factor; the moments hold the magnitude itself (m = 0.1 g, v = 0.001 g^2 after the first step).

MOMENT_TILE = 32


def tile_norms(a, tile=MOMENT_TILE):
    """L2 norm (float64) of every tile x tile tile of the 2-D array a: row and column tiles from index 0, edge tiles
    partial.  -> [ceil(rows / tile), ceil(cols / tile)]"""
    a = np.asarray(a, np.float64)
    r, c = a.shape
    nr, nc = -(-r // tile), -(-c // tile)
    sq = np.zeros((nr * tile, nc * tile))
    sq[:r, :c] = a * a
    return np.sqrt(sq.reshape(nr, tile, nc, tile).sum(axis=(1, 3)))


def _rel(num, den):
    """num / den elementwise; where the reference norm den is 0 the other side has to be exactly 0 as well (-> 0, else
    inf)."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))


def moments_err(got, ref):
    """Two dicts in the export_adam() / O.zeros_like_trainable format (one moment each) ->
    per tensor: {"gamma", "beta", "W<l>", "b<l>"} -> ||got - ref||_2 / ||ref||_2 in float64;
    per tile:   {"W<l>"} -> the worst value of the same ratio over the 32 x 32 tiles of W[l] (a tensor-wide norm would
                dilute a wrong k-tile or unit tile at the end of K or H)."""
    f64 = lambda a: np.asarray(a, np.float64)
    named = [("gamma", got["gamma"], ref["gamma"]), ("beta", got["beta"], ref["beta"])]
    for l in range(len(ref["W"])):
        named += [(f"W{l}", got["W"][l], ref["W"][l]), (f"b{l}", got["b"][l], ref["b"][l])]
    per_tensor, per_tile = {}, {}
    for name, g, r in named:
        assert np.shape(g) == np.shape(r), (name, np.shape(g), np.shape(r))
        per_tensor[name] = float(_rel(np.linalg.norm(f64(g) - f64(r)), np.linalg.norm(f64(r))))
        if name[0] == "W":
            per_tile[name] = float(_rel(tile_norms(f64(g) - f64(r)), tile_norms(r)).max())
    return per_tensor, per_tile


def replay_epoch(p, x, y, rows, batch, masks, drop_p, dtype=np.float64, grad_hook=None):
    """One epoch of O.train_step (Adam t = 1.., lr 1e-3, moments from zero) in `dtype` on the minibatches
    rows[j * batch:(j + 1) * batch] with the keep masks masks[j] ([rows of the step or more][mask width or more]).
    grad_hook(g) may edit the gradients before Adam sees them (the sensitivity tests of tests/test_oracle.py).
    -> per-step losses, m, v; p itself is left alone."""
    pr = O.cast_params(p, dtype)
    m, v = O.zeros_like_trainable(pr), O.zeros_like_trainable(pr)
    nl = len(pr["W"]) - 2
    mw = pr["W"][0].shape[0] if O.n_pre(nl) == 0 else pr["W"][0].shape[1]
    losses = []
    for j, i in enumerate(range(0, len(rows), batch)):
        r = rows[i:i + batch]
        mask = masks[j][:len(r), :mw] if drop_p > 0 else None
        loss, g, _ = O.loss_and_grads(pr, x[r], y[r], mask, drop_p)
        if grad_hook is not None:
            grad_hook(g)
        O.adam_apply(pr, g, m, v, j + 1, dtype(1e-3))
        losses.append(float(loss))
    return np.array(losses), m, v


def moments_padding(net, flat):
    """Entries of the flat adam_m / adam_v buffer that belong to no trainable value: W1 rows K..Kp and units H..Hp (W1S
    layout), gamma / beta beyond K, b1 / hidden biases beyond H, hidden rows and columns H..Hp, head rows H..Hp and the
    alignment tail.  -> the values found there (all of them have to be 0)."""
    d, lay = net.d, net.lay
    K, Kp, H, Hp, L = d.K, d.Kp, d.H, d.Hp, d.L
    flat = flat.cpu().numpy()
    assert flat.size == lay.n_trainable
    real = np.zeros(flat.size, bool)
    idx = _w1s_tile_index(Hp)                                         # [32, Hp] offsets inside one k-tile's run
    for kt in range(Kp // 32):
        ok = ((32 * kt + np.arange(32))[:, None] < K) & (np.arange(Hp)[None, :] < H)
        real[lay.w1 + kt * 32 * Hp + idx[ok]] = True
    real[lay.gamma:lay.gamma + K] = True
    real[lay.beta:lay.beta + K] = True
    real[lay.b1:lay.b1 + H] = True
    sq = np.zeros((Hp, Hp), bool)
    sq[:H, :H] = True
    for i in range(L - 1):
        real[lay.wh + i * Hp * Hp:lay.wh + (i + 1) * Hp * Hp] = sq.reshape(-1)
        real[lay.bh + i * Hp:lay.bh + i * Hp + H] = True
    real[lay.wa:lay.wa + 2 * H] = True                                # [Hp][2]: rows H..Hp are padding
    real[lay.ba:lay.ba + 2] = True
    real[lay.wb:lay.wb + 4] = True
    real[lay.bb:lay.bb + 2] = True
    assert real.sum() == K * H + 2 * K + H + (L - 1) * (H * H + H) + 2 * H + 2 + 4 + 2
    return flat[~real]


# ---------------------------------------------------------------- sparse-support problems (tests/test_gpu_large_k.py)
# Only a few 32-SNP k-tiles carry real genotypes and keep their first-layer weights; every other SNP column is constant
# over the samples (mostly 0, one tile of 1s and one of 2s) and its W1 row is zero.  There x - mean = 0 exactly, so those
# columns add nothing to z1, their W1 / gamma / beta gradients are exactly 0 (dbeta_k = sum_h (sum_b dZ_bh) W1_kh) and
# Adam leaves W1 / m / v / gamma / beta bit-for-bit where they were: the full problem trains exactly like the REDUCED one
# made of the active columns alone (tests/test_oracle.py pins this on the oracle), which the fp64 oracle can afford at
# millions of SNPs.  Nothing here builds a K x H array, on the device or the host.

def sparse_problem(K, width, nlayers, active_tiles, n, seed):
    """-> x (n, K) uint8, y (n, 2), cols (sorted active SNP columns < K), const {tile: value} of the 1s / 2s tiles.
    Each active tile draws its own allele frequencies, so reading the wrong tile changes the numbers."""
    rng = np.random.default_rng(seed)
    nkt = (K + 31) // 32
    tiles = sorted(set(int(t) for t in active_tiles))
    assert tiles and tiles[0] >= 0 and tiles[-1] < nkt, (tiles, nkt)
    x = np.zeros((n, K), np.uint8)
    for kt in tiles:
        k0, k1 = 32 * kt, min(32 * kt + 32, K)
        af = rng.beta(0.4, 0.9, k1 - k0).clip(0.05, 0.95)
        x[:, k0:k1] = rng.binomial(2, af, (n, k1 - k0))
    free = [kt for kt in (2, 3, nkt - 2, nkt - 3) if 0 <= kt < nkt and kt not in tiles]
    const = {free[0]: 1, free[-1]: 2} if len(free) >= 2 else {}
    for kt, c in const.items():
        x[:, 32 * kt:min(32 * kt + 32, K)] = c
    cols = np.concatenate([np.arange(32 * kt, min(32 * kt + 32, K)) for kt in tiles])
    xa = x[:, cols].astype(np.float64)
    y = (xa - xa.mean(0)) @ (rng.normal(0, 1, (len(cols), 2)) / np.sqrt(len(cols)))
    y = (y - y.mean(0)) / y.std(0)
    return x, y, cols, const


def keep_w1_tiles(net, tiles):
    """Zero every W1 row of the device-initialised net except the k-tiles `tiles`: in the W1S layout k-tile kt is the
    contiguous run of 32 * Hp floats at lay.w1 + kt * 32 * Hp, so the runs are saved, the section zeroed, the runs
    written back."""
    run = 32 * net.d.Hp
    w1 = net.params[net.lay.w1:net.lay.w1 + net.d.Kp * net.d.Hp]
    saved = [w1[kt * run:(kt + 1) * run].clone() for kt in tiles]
    w1.zero_()
    for kt, s in zip(tiles, saved):
        w1[kt * run:(kt + 1) * run] = s
    net.params_changed()


def _w1s_tile_index(Hp):
    """[32, Hp] offsets of (SNP kl, unit h) inside one k-tile's run of the W1S layout (loc_w1s_index with kt = 0)."""
    kl, h = np.meshgrid(np.arange(32), np.arange(Hp), indexing="ij")
    ht, hl = h >> 5, h & 31
    q, hi, c = hl >> 3, (hl >> 2) & 1, hl & 3
    return ((ht * 4 + q) * 256 + (hi * 32 + kl) * 4 + c).astype(np.int64)


def read_w1_tiles(flat, lay, tiles, Hp):
    """(32 * len(tiles), Hp) rows of W1 (or of its Adam moments: same layout) for the k-tiles `tiles`, in Keras
    orientation, read from the flat device buffer tile by tile."""
    run = 32 * Hp
    idx = _w1s_tile_index(Hp)
    out = [flat[lay.w1 + kt * run:lay.w1 + (kt + 1) * run].cpu().numpy()[idx] for kt in tiles]
    return np.concatenate(out, 0)


def export_reduced(net, flat, tiles, cols, with_moving=True):
    """Oracle-format dict of the reduced problem from a flat device buffer (params, adam_m or adam_v): W[0] = the W1 rows
    of the active SNPs `cols` (k-tiles `tiles`), gamma / beta / moving statistics at those SNPs; hidden layers and heads
    straight from their small sections."""
    d, lay = net.d, net.lay
    rows = np.concatenate([np.arange(32 * kt, 32 * kt + 32) for kt in tiles])
    keep = np.isin(rows, cols)
    W = [read_w1_tiles(flat, lay, tiles, d.Hp)[keep][:, :d.H]]
    b = [flat[lay.b1:lay.b1 + d.H].cpu().numpy()]
    for i in range(d.L - 1):
        W.append(flat[lay.wh + i * d.Hp * d.Hp:lay.wh + (i + 1) * d.Hp * d.Hp].view(d.Hp, d.Hp)[:d.H, :d.H].cpu().numpy())
        b.append(flat[lay.bh + i * d.Hp:lay.bh + i * d.Hp + d.H].cpu().numpy())
    W.append(flat[lay.wa:lay.wa + 2 * d.Hp].view(d.Hp, 2)[:d.H].cpu().numpy())
    b.append(flat[lay.ba:lay.ba + 2].cpu().numpy())
    W.append(flat[lay.wb:lay.wb + 4].view(2, 2).cpu().numpy())
    b.append(flat[lay.bb:lay.bb + 2].cpu().numpy())
    sel = torch.from_numpy(cols.astype(np.int64)).to(flat.device)
    out = {"W": W, "b": b}
    for k in ("gamma", "beta") + (("mov_mean", "mov_var") if with_moving else ()):
        out[k] = flat[getattr(lay, k) + sel].cpu().numpy()
    return out


def untouched(section, tiles, value, per_tile, atol=0.0, chunk=1 << 26):
    """Entries of `section` (a flat device view, per_tile entries per k-tile) OUTSIDE the k-tiles `tiles` that differ from
    `value` by more than atol, counted on the device chunk by chunk (no copy of the section)."""
    bad, start = 0, 0
    for end in sorted(int(t) * per_tile for t in tiles) + [section.numel()]:
        for a in range(start, end, chunk):
            part = section[a:min(a + chunk, end)]
            bad += int(((part != value) if atol == 0 else ((part - value).abs_() > atol)).sum().item())
        start = max(start, end + per_tile)
    return bad


def w1s_pack(w_kh, Kp, Hp):
    """[K][H] (Keras orientation, K <= Kp, H <= Hp) -> the flat W1S array of Kp * Hp fp32 values, padding zero."""
    w_kh = np.asarray(w_kh, np.float32)
    full = np.zeros((Kp, Hp), np.float32)
    full[:w_kh.shape[0], :w_kh.shape[1]] = w_kh
    idx = _w1s_tile_index(Hp)
    out = np.empty(Kp * Hp, np.float32)
    for kt in range(Kp // 32):
        out[kt * 32 * Hp + idx] = full[32 * kt:32 * kt + 32]
    return out


def w1s_unpack(flat, Kp, Hp):
    """The inverse: flat W1S array (W1 or one of its Adam moments) -> [Kp][Hp], padding included."""
    flat = np.asarray(flat)
    assert flat.size == Kp * Hp, (flat.size, Kp, Hp)
    idx = _w1s_tile_index(Hp)
    return np.concatenate([flat[kt * 32 * Hp:(kt + 1) * 32 * Hp][idx] for kt in range(Kp // 32)], 0)


def ulp32(a):
    """Spacing of the fp32 numbers at |a| (float64 array): the unit in which "within n ulp" is counted."""
    a = np.abs(np.asarray(a, np.float64)).astype(np.float32)
    return np.spacing(np.maximum(a, np.float32(1.1754944e-38))).astype(np.float64)
