"""What tests/test_gptq_walk_cpu.py and tests/test_gptq_walk_gpu.py share: `walk`, a numpy float32 restatement of the column walk of
csrc/gptq_quant.hip and csrc/gptq_static.hip (one rounding per product, sum, difference and quotient, the kernels' order of every
sum), the case matrix, and the inputs of a case.  Nothing here calls the library: numpy and torch only.

The kernels fix the order of every floating-point operation themselves, so their outputs are a function of the inputs
that can be restated operation by operation; the tests compare bits."""
import zlib

import numpy as np
import torch

F = np.float32
BLK = 128          # the reference's blocksize; when group parameters are found depends on it
TINY = 2.0 ** -100  # no nonzero w / acc / ev of a case may be smaller: subnormal handling stays out of the comparison
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}


def find_params(mn, mx, maxq, sym):
    """scale, zero of groups whose minimum / maximum (already taken against 0) are mn / mx (float32 arrays of one shape)."""
    if sym:
        mx = np.maximum(np.abs(mn), mx)
        mn = np.where(mn < 0, -mx, mn)
    flat = (mn == 0) & (mx == 0)
    mn, mx = np.where(flat, F(-1), mn), np.where(flat, F(1), mx)
    scale = (mx - mn) / maxq
    zero = np.full_like(scale, (maxq + F(1)) * F(0.5)) if sym else np.rint(-mn / scale)
    return scale.astype(F), zero.astype(F)


def group_table(w, g, maxq, sym):
    """find_params of every whole group of g columns of w [N, n * g]: two [N, n] arrays."""
    v = w.reshape(w.shape[0], -1, g)
    return find_params(np.minimum(v.min(2), F(0)), np.maximum(v.max(2), F(0)), maxq, sym)


def lane_of(i):
    """The lane of a row's 16 that owns column i of a 128-column block: columns 4l..4l+3 and 64+4l..64+4l+3."""
    return (i % 64) // 4


def _note(stats, key, *arrays):
    """stats[key]: the smallest nonzero magnitude seen so far."""
    if stats is None:
        return
    for a in arrays:
        nz = np.abs(a[a != 0])
        if nz.size:
            stats[key] = min(stats.get(key, np.inf), float(nz.min()))


def walk(W, U, perm, bits, g, sym, static, stats=None):
    """W [N, K] float32 (the dynamic kernel: columns in processing order; the static one: in the original order), U [K, K] float32 in
    processing order or None, perm [K] (static only: processing position -> original column) or None
    -> codes [N, K] int32, scale [N, K/g], zero [N, K/g], dq [N, K], err [N, K], loss [N], all float32 but the codes.
    codes and dq lie where the kernel stores them (static: at the original column), err in processing order, every block included.
    `stats`, a dict, receives the smallest nonzero |w|, |acc|, |ev| ("tiny") and |product| ("product") of the run."""
    W = np.ascontiguousarray(W)
    N, K = W.shape
    assert W.dtype == F and (U is None or U.dtype == F) and K % g == 0
    G, maxq = K // g, F(2 ** bits - 1)
    if U is None:
        perm = None                                             # u == NULL: the order has no effect, perm is not consulted
    assert perm is None or static
    col_of = np.arange(K) if perm is None else np.asarray(perm, dtype=np.int64)
    shift = 31 if g == K else g.bit_length() - 1
    Wp = W[:, col_of]
    if static or g == K:
        scale, zero = group_table(W, g, maxq, sym)              # from the original columns c*g .. c*g+g-1
    else:
        scale, zero = np.zeros((N, G), F), np.zeros((N, G), F)  # found block by block
    codes, dq, err = np.zeros((N, K), np.int32), np.zeros((N, K), F), np.zeros((N, K), F)
    lanes = np.zeros((N, 16), F)                                # the loss of a row as its 16 lanes hold it

    for i1 in range(0, K, BLK):
        cnt = min(BLK, K - i1)
        w = Wp[:, i1:i1 + cnt].copy()
        if U is not None:
            for p1 in range(0, i1, BLK):                        # every earlier block, ascending
                acc = np.zeros((N, cnt), F)
                for k in range(p1, p1 + BLK):
                    prod = err[:, k, None] * U[None, k, i1:i1 + cnt]
                    acc = acc + prod
                    _note(stats, "product", prod)
                w = w - acc
                _note(stats, "tiny", acc, w)
        if not static and g != K:                               # the dynamic kernel: from the block-boundary state
            s, z = group_table(w, g, maxq, sym)
            scale[:, i1 // g:i1 // g + cnt // g], zero[:, i1 // g:i1 // g + cnt // g] = s, z
        grp = (col_of[i1:i1 + cnt] >> shift) if static else (np.arange(i1, i1 + cnt) >> shift)
        _note(stats, "tiny", w)
        for i in range(cnt):
            s, z = scale[:, grp[i]], zero[:, grp[i]]
            x = w[:, i]
            q = np.minimum(np.maximum(np.rint(x / s) + z, F(0)), maxq)
            y = s * (q - z)
            diff = x - y
            if U is None:
                ev, term = np.zeros(N, F), diff * diff
            else:
                d = U[i1 + i, i1 + i]
                ev = diff / d
                term = (diff * diff) / (d * d)
                prod = ev[:, None] * U[None, i1 + i, i1 + i + 1:i1 + cnt]
                w[:, i + 1:] = w[:, i + 1:] - prod
                _note(stats, "product", prod)
                _note(stats, "tiny", ev, w[:, i + 1:])
            lanes[:, lane_of(i)] = lanes[:, lane_of(i)] + term  # a lane meets its columns in ascending order, block after block
            codes[:, col_of[i1 + i]], dq[:, col_of[i1 + i]], err[:, i1 + i] = q.astype(np.int32), y, ev
    for m in (1, 2, 4, 8):                                      # the xor butterfly over the row's lanes
        lanes = lanes + lanes[:, np.arange(16) ^ m]
    loss = lanes[:, 0] * F(0.5)
    for a in (scale, zero, dq, err, loss):
        assert a.dtype == F
    return codes, scale, zero, dq, err, loss


# ---- the case matrix ----------------------------------------------------------------------------------------------------------------------
def case(kernel, N, K, g, bits=4, sym=0, dtype="float16", w="randn", u="dense", perm="none"):
    c = dict(kernel=kernel, N=N, K=K, g=g, bits=bits, sym=sym, dtype=dtype, w=w, u=u, perm=perm)
    c["id"] = f"{kernel}-N{N}-K{K}-g{'K' if g == K else g}-w{bits}{'s' if sym else 'a'}-{dtype}-{w}-{u}" + ("" if perm == "none" else "-" + perm)
    return c


def _dynamic():
    out = [case("dyn", 17, 384, 64, bits, sym, "float32") for bits in range(2, 9) for sym in (0, 1)]            # widths
    for K, gs in ((128, (32, 64, 128)), (160, (32, 160)), (192, (32, 64, 192)), (320, (32, 64, 320)), (416, (32, 416)),
                  (1024, (32, 64, 128, 1024))):                                                                   # groups and K
        out += [case("dyn", 40, K, g) for g in gs]
    # one group per row (K = 4: two of a row's four values are its extremes, so 8 bits for the update to move a code of the others)
    out += [case("dyn", 17, K, K, 8 if K == 4 else 4) for K in (4, 100, 252, 640)]
    out += [case("dyn", N, 320, 64) for N in (1, 15, 16, 17)]                                                    # rows (N = 40: above)
    out += [case("dyn", 17, 192, g, 4, sym, dt) for dt in DTYPES for g in (32, 192) for sym in (0, 1)]           # storage
    out += [case("dyn", 17, 320, 64, w=w) for w in ("signed", "flat", "outlier", "dead")]                        # values
    out += [case("dyn", 17, 320, g, bits, w="ties", u="none") for g, bits in ((64, 4), (32, 3), (320, 8))]
    out += [case("dyn", 17, 320, 64, u=u) for u in ("none", "identity", "diag")]                                 # factors
    return out


def _static():
    perms = ("none", "reversed", "random", "diag")
    out = [dict(c, kernel="static", perm=perms[i % 4] if c["u"] == "dense" else "none") for i, c in enumerate(_dynamic()[::2])]
    out += [case("static", 17, 256, 32, perm="random"), case("static", 40, 416, 32, perm="random"),              # eight groups in a lane
            case("static", 17, 320, 64, w="outlier", perm="diag"), case("static", 17, 320, 64, w="flat", perm="reversed"),
            case("static", 17, 320, 64, w="signed", perm="random"), case("static", 17, 252, 252, perm="random"),
            case("static", 17, 320, 64, u="identity"), case("static", 17, 320, 64, u="none", perm="random"),
            case("static", 1, 320, 64, perm="reversed"), case("static", 16, 320, 64, 4, 1, "bfloat16", perm="diag"),
            case("static", 17, 384, 64, 5, 1, "float32", perm="diag"), case("static", 17, 192, 32, 8, 0, "bfloat16", perm="random")]
    return [case(**{k: v for k, v in c.items() if k != "id"}) for c in out]


DYNAMIC, STATIC = _dynamic(), _static()
CASES = DYNAMIC + STATIC
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
DEAD = lambda K: [5, K // 2, K - 1]      # the dead input channels of a "dead" case

_cache = {}


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def hessian(K):
    """float64 H [K, K] of 2048 activations with unequal channel scales (the recipe of the dynamic file's N = 1000 test) that share a
    common component, so that every channel is correlated with every other and U is dense in earnest even at K = 4."""
    if ("H", K) not in _cache:
        gen = torch.Generator().manual_seed(_seed("H", K))
        X = torch.randn((2048, K), generator=gen) + 0.5 * torch.randn((2048, 1), generator=gen)
        X = X * torch.exp(0.5 * torch.randn(K, generator=gen))
        _cache["H", K] = (2.0 / 2048 * X.T @ X).double()
    return _cache["H", K]


def factor(K, dead, order):
    """The float32 upper Cholesky factor of the inverse of H[order][:, order], H with its dead channels cleared and its diagonal damped
    by 1 % of its mean, as gptq_quantize_weight prepares it."""
    key = ("U", K, dead, tuple(order.tolist()))
    if key not in _cache:
        H = hessian(K).clone()
        if dead:
            H[DEAD(K), :] = 0
            H[:, DEAD(K)] = 0
            H[DEAD(K), DEAD(K)] = 1
        H = H[order][:, order]
        H += 0.01 * H.diag().mean() * torch.eye(K, dtype=torch.float64)
        U = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H)), upper=True)
        _cache[key] = np.ascontiguousarray(U.float().numpy())
    return _cache[key]


def ties(N, K, g, bits, gen):
    """Every group holds 0 and maxq (scale exactly 1) and otherwise k + 0.5 with even and odd k: each rounding is an exact tie."""
    maxq = 2 ** bits - 1
    W = torch.randint(0, maxq, (N, K), generator=gen).float() + 0.5
    W[:, 0::g], W[:, 1::g] = 0.0, float(maxq)
    W[:, 2::g], W[:, 3::g] = 0.5, 1.5                      # an even and an odd k in every group, whatever the draw
    return W


def inputs(c):
    """(W [N, K] float32 numpy with every value exact in the case's storage type, U [K, K] float32 numpy or None, perm int64 [K] or None).
    Dynamic cases: W is in processing order and perm is None."""
    N, K, g, bits, dt = c["N"], c["K"], c["g"], c["bits"], DTYPES[c["dtype"]]
    gen = torch.Generator().manual_seed(_seed(c["id"]))
    W = 0.02 * torch.randn((N, K), generator=gen)
    grp = torch.arange(K) // g
    rows = torch.arange(N)
    if c["w"] == "signed":          # one-signed groups: all positive (zero = 0) and all negative (zero = maxq) alternate
        W = W.abs() * torch.where((rows[:, None] + grp[None, :]) % 2 == 0, 1.0, -1.0)
    elif c["w"] == "flat":          # a flat group in every row (group n mod G: group 0, found from the original W, in some rows) ...
        W[grp[None, :] == (rows[:, None] % (K // g))] = 0
        W[0] = 0                    # ... and an all-zero row
    elif c["w"] == "outlier":       # 50 sigma
        W[rows, (7 * rows + 3) % K] = torch.where(rows % 2 == 0, 1.0, -1.0)
    elif c["w"] == "dead":
        W[:, DEAD(K)] = 0
    elif c["w"] == "ties":
        W = ties(N, K, g, bits, gen)
    W = W.to(dt).float() + 0.0                                            # (-0 + 0 = +0: a draw that underflows leaves no -0 ...
    assert not bool(((W == 0) & torch.signbit(W)).any())                  # ... since fminf(-0, +0) may return either)
    perm = {"none": None, "reversed": np.arange(K)[::-1].copy(), "random": torch.randperm(K, generator=gen).numpy(),
            "diag": None}[c["perm"]]
    if c["perm"] == "diag":         # act-order: descending diag(H), dead channels as 1
        dg = hessian(K).diag().numpy().copy()
        if c["w"] == "dead":
            dg[DEAD(K)] = 1
        perm = np.argsort(-dg, kind="stable")
    assert perm is None or c["kernel"] == "static"
    if c["u"] == "none":
        U = None
    elif c["u"] == "identity":
        U = np.eye(K, dtype=F)
    elif c["u"] == "diag":
        U = np.diag((0.5 + 1.5 * torch.rand(K, generator=gen)).numpy().astype(F))
    else:
        U = factor(K, c["w"] == "dead", np.arange(K) if perm is None else perm)
    return W.numpy(), U, perm


def run(c, stats=None):
    """The oracle's outputs of a case (computed once per process and shared: treat them as read-only)."""
    if stats is not None or c["id"] not in _cache:
        W, U, perm = inputs(c)
        out = walk(W, U, perm, c["bits"], c["g"], bool(c["sym"]), c["kernel"] == "static", stats)
        if stats is not None:
            return out
        _cache[c["id"]] = out
    return _cache[c["id"]]
