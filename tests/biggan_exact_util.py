"""Generators and float64 references for the exact-arithmetic tests of the attention, spectral-norm, minibatch-std and grouped-GEMM kernels
(tests/test_biggan_exact_gpu.py; the preconditions every case rests on are asserted without a device in tests/test_biggan_exact_cases_cpu.py).
Everything here is float64 on the CPU; the exact-mode rules are those of exact_util.py.

Attention, "selection" construction.  Key k carries the code c(k) in {-1, +1}^B of its binary digits (times a per-sample sign pattern):
phi[k, :B] = c(k), phi[k, B] = 1.  Query q with target key t(q): theta[q, :B] = 64 c(t(q)) with the dimensions in Z zeroed, theta[q, B] =
-64 (B - |Z|).  (The B + 1 dimensions are spread evenly over the D columns, the rest of which are zero.)  Every key that agrees with t(q) outside Z has logit exactly 0, every other key is lower by 128 per differing digit, so in fp32
exp(logit - max) is exactly 1 on the tie set and exactly 0 elsewhere: P = 2^-j on 2^j keys.  g and dout are small integers."""
import math

import numpy as np
import torch

from exact_util import qint

# ---------------------------------------------------------------------------------------------------------------- attention

ATT_CHUNK = 128            # keys per chunk of the streamed kernels (csrc/biggan_ops.hip)
ATT_MAX_M = 256            # above it the streamed kernels run
TILE_COUNTS = (1, 2, 4, 8, 16)


def code_bits(m):
    return max(1, int(math.ceil(math.log2(m))))


def min_d(m):
    """the smallest multiple of 4 holding the B code dimensions and the shift dimension"""
    return (code_bits(m) + 1 + 3) // 4 * 4


def z_sets(m, where):
    """the zeroed code dimensions of the three modes |Z| = 0, 1, 2.  'high': the top digit (tie sets straddle the halves of the key range:
    chunks of 128 and tiles of 16, and for M = 256 + 16 / 512 + 16 the 16-key remainder chunk); 'low': digits 0 / 1 and 4 (neighbours, and
    the next 16-key tile).  M that is no power of two takes the top digit only together with digit 0, so that every tie count stays 2^j."""
    b = code_bits(m)
    pow2 = m == 1 << b
    if where == "high":
        return [(), (b - 1,), (b - 1, b - 2) if pow2 and b >= 2 else (b - 1, 0)]
    return [(), (0,), (1, 4) if b > 4 else (1, 2)]


def att_targets(n, q, m, gen):
    """t[s, q] = perm_s[q mod M]: a permutation of the keys per sample whose first entries are forced to the edges of the key range, of the
    16-key tiles and of the 128-key chunks (so that with Q = 16 rows win in the first chunk, in the last chunk and in a remainder chunk)"""
    forced = []
    for k in (0, m - 1, m - 16, 15, 16 % m, 127 % m, 128 % m, (m - 17) % m, m // 2, m // 2 - 1):
        if k not in forced:
            forced.append(k)
    out = []
    for s in range(n):
        lead = forced[s:] + forced[:s]
        rest = [k for k in torch.randperm(m, generator=gen).tolist() if k not in forced]
        perm = torch.tensor(lead + rest)
        assert sorted(perm.tolist()) == list(range(m))
        out.append(perm[torch.arange(q) % m])
    return torch.stack(out)


def att_case(n, q, m, d, dv, z=(), seed=0, shift=True, gaussian_g=False):
    """-> dict(theta [n,q,d], phi [n,m,d], g [n,m,dv], dout [n,q,dv], targets [n,q], z)"""
    b = code_bits(m)
    assert d % 4 == 0 and d >= b + (1 if shift else 0) and all(0 <= i < b for i in z)
    gen = torch.Generator().manual_seed(1000 + seed)
    targets = att_targets(n, q, m, gen)
    digits = ((torch.arange(1 << b).unsqueeze(1) >> torch.arange(b)) & 1).double() * 2 - 1          # [2^B, B]
    sign = (torch.randint(0, 2, (n, 1, b), generator=gen) * 2 - 1).double()                        # a sign pattern per sample: the logits
    phi = torch.zeros(n, m, d, dtype=torch.float64)                                                # do not change, the operands do
    theta = torch.zeros(n, q, d, dtype=torch.float64)
    ndim = b + (1 if shift else 0)
    pos = [(i * d) // ndim for i in range(ndim)]               # the code (and shift) dimensions spread over [0, D): every 16-column tile of a
    if z:                                                      # wide D carries some, the spare dimensions between them are zero; rotated so
        pos = [(c + d - 1 - pos[z[0]]) % d for c in pos]       # that the first zeroed digit -- dtheta is nonzero only on Z -- is column D - 1
    assert len(set(pos)) == ndim
    keep = torch.ones(b, dtype=torch.float64)
    keep[list(z)] = 0
    phi[:, :, pos[:b]] = digits[:m].unsqueeze(0) * sign
    theta[:, :, pos[:b]] = 64 * digits[targets] * sign * keep
    if shift:
        phi[:, :, pos[b]] = 1
        theta[:, :, pos[b]] = -64 * (b - len(z))
    g = torch.randn(n, m, dv, generator=gen).float().double() if gaussian_g else qint(gen, (n, m, dv))
    dout = qint(gen, (n, q, dv))
    return dict(theta=theta, phi=phi, g=g, dout=dout, targets=targets, z=tuple(z), shape=(n, q, m, d, dv))


def att_terms(case):
    """the factors of the forward and the first-order backward in float64, with the softmax as fp32 arithmetic sees it: S, P, out, dP, delta, dS, dtheta, dphi, dg, and A_* = the same
    gradient expressions with the absolute value of every factor (the scale of the element-wise bounds)"""
    t, p, g, do = case["theta"], case["phi"], case["g"], case["dout"]
    S = t @ p.transpose(1, 2)
    mx = S.max(-1, keepdim=True).values
    win = (S == mx).double()                     # fp32: exp(s - max) is 1 on the winners and exactly 0 at a gap of 128 or more (float64 keeps
    P = win / win.sum(-1, keepdim=True)          # 2.6e-56 there, which no fp32 result can show: the CPU test bounds that difference)
    out = P @ g
    dP = do @ g.transpose(1, 2)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    A_dP = do.abs() @ g.abs().transpose(1, 2)
    A_dS = P * (A_dP + (P * A_dP).sum(-1, keepdim=True))
    return dict(S=S, mx=mx, P=P, out=out, dP=dP, delta=delta, dS=dS, dtheta=dS @ p, dphi=dS.transpose(1, 2) @ t, dg=P.transpose(1, 2) @ do,
                A_dtheta=A_dS @ p.abs(), A_dphi=A_dS.transpose(1, 2) @ t.abs(), A_dg=P.transpose(1, 2) @ do.abs(), A_dS=A_dS)


def att_two_pass_f32(case):
    """float32 numpy restatement of the backward as the per-key-tile pass and the streamed dtheta pass formulate it: lse = max + log(sum),
    P = exp(S - lse), dS = P o (dP - delta), everything float32.  A reference for the size of the rounding of that formulation (the constant c
    of the tied-row bounds), not the code under test."""
    f = np.float32
    t, p, g, do = [case[k].numpy().astype(f) for k in ("theta", "phi", "g", "dout")]
    S = np.matmul(t, p.transpose(0, 2, 1))
    mx = S.max(-1, keepdims=True)
    E = np.exp(S - mx)
    ssum = E.sum(-1, keepdims=True, dtype=f)
    lse = (mx + np.log(ssum)).astype(f)
    P = np.exp((S - lse).astype(f)).astype(f)
    dP = np.matmul(do, g.transpose(0, 2, 1))
    delta = ((E / ssum) * dP).sum(-1, keepdims=True, dtype=f)
    dS = (P * (dP - delta)).astype(f)
    return dict(dtheta=np.matmul(dS, p), dphi=np.matmul(dS.transpose(0, 2, 1), t), dg=np.matmul(P.transpose(0, 2, 1), do))


def bound_ratio(got, ref64, scale):
    """max over the elements of |got - ref64| / (2^-24 scale); an element whose scale is 0 must be exact (ratio inf otherwise)"""
    got = torch.as_tensor(got).detach().cpu().double()
    err = (got - ref64).abs()
    zero = scale == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    return float((err[~zero] / (2.0 ** -24 * scale[~zero])).max()) if bool((~zero).any()) else 0.0


def pow2_ceil(x):
    """the smallest power of two >= x (0 for x = 0)"""
    return 0.0 if x <= 0 else 2.0 ** math.ceil(math.log2(x))


# The constant c of the tied-row bounds |got - ref64| <= c 2^-24 A: 4x the worst ratio att_two_pass_f32 reaches over ATT_CASES, rounded up to
# a power of two (tests/test_biggan_exact_cases_cpu.py recomputes it).  The restatement reaches ratio 0: log(2^j) rounded to float32 and
# exp of its negative round back to exactly 2^-j for j = 1, 2 when both functions are correctly rounded, so P and every sum stay exact.
# c = 0 therefore asks the device for the exact gradients on tied rows as well.
ATT_TIED_C = 0.0


def att_instantiations(variant, dims):
    """the kernel template instantiations a launch record of kind "attention" stands for (dispatch of csrc/biggan_ops.hip: MT = M / 16, DT =
    ceil(D / 16), DVT = DV / 16 in the backward, the largest of 16, 8, 4, 2, 1 dividing DV / 16 in the streamed forward)"""
    n, q, m, d, dv, backward = dims[:6]
    dt, dvt = (d + 15) // 16, dv // 16
    if variant == "single":
        return [f"dq<MT={m // 16}>", f"dkv<DVT={dvt},DT={dt}>"] if backward else [f"fwd<MT={m // 16}>"]
    if variant == "stream":
        f = 16
        while dvt % f:
            f //= 2
        return [f"stream<DVT={f},STATS=0>"]
    return {"stream_stats": [f"stream<DVT={dvt},STATS=1>"], "stream_dq": [f"dq_stream<DT={dt}>"], "stream_dkv": [f"dkv<DVT={dvt},DT={dt}>"]}[variant]


ALL_INSTANTIATIONS = sorted([f"fwd<MT={t}>" for t in TILE_COUNTS] + [f"dq<MT={t}>" for t in TILE_COUNTS]
                            + [f"stream<DVT={t},STATS={s}>" for t in TILE_COUNTS for s in (0, 1)] + [f"dq_stream<DT={t}>" for t in (1, 2, 4)]
                            + [f"dkv<DVT={v},DT={t}>" for v in TILE_COUNTS for t in (1, 2, 4)])


def _att_case_table():
    """(q, m, d, dv, where) with n = 2 throughout"""
    table = []
    i = 0
    for m in (16, 32, 64, 128, 256):                  # single chunk: every MT, both Q, DV 16 / 48 (forward only: three tiles) / 256
        for q in (16, 80):
            for dv in (16, 48, 256):
                table.append((q, m, min_d(m), dv, ("high", "low")[i % 2])); i += 1
    for m in (272, 512, 528, 1024):                   # streamed: every DVT with and without the statistics, grid.z = 3 at DV 48
        for dv in (16, 32, 48, 64, 128, 256):
            table.append(((16, 80)[i % 2], m, min_d(m), dv, ("high", "low")[(i // 2) % 2])); i += 1
    ms = (32, 272, 528, 128, 16, 512, 1024, 64, 256, 272)
    for j, (dv, d) in enumerate((dv, d) for dv in (16, 32, 64, 128, 256) for d in (24, 64)):     # DT = 2 and 4 against every DVT
        table.append(((80, 16)[j % 2], ms[j], d, dv, ("high", "low")[j % 2]))
    return table


ATT_CASES = _att_case_table()
ATT_ONE_HOT_NO_SHIFT = (16, 16, 4, 16)               # D = 4 holds the four code digits and no shift dimension: the row maximum is 256


def att_case_id(c):
    return "x".join(map(str, c[:4])) + "-" + c[4]


# ---------------------------------------------------------------------------------------------------------------- spectral norm

def hadamard(n):
    """Sylvester's Hadamard matrix of order n = 2^k (entries +-1, rows orthogonal, row norm sqrt(n)), float64"""
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == n
    return h


SN_EXACT_CASES = [(33, 256), (64, 256), (33, 1024), (64, 1024)]
SN_EXACT_EXPONENTS = (-3, 0, 5)


def sn_exact_case(rows, cols, seed=0):
    """W = `rows` distinct rows of the Hadamard matrix of order cols (a seeded choice, in a seeded order)"""
    pick = torch.randperm(cols, generator=torch.Generator().manual_seed(50 + seed))[:rows]
    return hadamard(cols)[pick].contiguous()


def sn_exact_rows(rows):
    """the rows i of u = 2^a e_i: the first, the last of the first 32-row block, the first of the second, one inside it, the last"""
    return sorted({0, 31, 32, rows // 2 + 7, rows - 1})


def sn_exact_expect(W, i, a):
    """(sigma, u_new, v) of one power iteration from u = 2^a e_i"""
    rows, cols = W.shape
    norm = math.sqrt(cols)
    assert norm == int(norm)
    u_new = torch.zeros(1, rows, dtype=torch.float64)
    u_new[0, i] = 1
    return torch.tensor(norm, dtype=torch.float64), u_new, (W[i] / norm).reshape(1, cols)


def sn_reference(W, u, eps=1e-12):
    """one power iteration as the reference composes it (F.normalize twice), in the dtype of its inputs -> (sigma, u_new, v)"""
    F = torch.nn.functional
    v = F.normalize(u @ W, eps=eps)
    t = v @ W.t()
    u_new = F.normalize(t, eps=eps)
    return (t @ u_new.t()).reshape([]), u_new, v


SN_SWEEP = [(r, c) for r in (1, 31, 32, 33, 65) for c in (1, 255, 256, 257, 513)] + [(1, 2048), (10, 128)]

# ---------------------------------------------------------------------------------------------------------------- minibatch std

MBSTD_EXACT = [(8, 64, 16, 4, 1), (8, 32, 16, 2, 2), (4, 512, 16, 4, 1), (4, 24, 16, 4, 3)]       # (N, C, HW, G, F)
MBSTD_RAGGED = (6, 20, 9, 3, 2)
MBSTD_SIGNS = {2: (1.0, -1.0), 3: (1.0, -1.0, 0.0), 4: (1.0, -1.0, -1.0, 1.0)}


def mbstd_case(shape, seed=0):
    """x[g M + m, ch, p] = a[m, ch, p] + s[g] d[m, ch, p], integer a, d in {1, 2, 4}, signs s summing to 0: the group mean is a, the group
    variance d^2 (G = 3: 2 d^2 / 3).  dy: small integers; where c HW G is a power of two the last element of every (m, f) group of the extra
    channel is set so that the group's sum is T c HW G with T in {-2, -1, 1, 2}.  -> dict(x, dy, a, d, s, T (None when ragged), hw side)"""
    N, C, HW, G, F = shape
    M, c, side = N // G, C // F, int(round(math.sqrt(HW)))
    assert side * side == HW
    gen = torch.Generator().manual_seed(300 + seed)
    a = qint(gen, (M, C, side, side), hi=8)
    d = torch.pow(2.0, torch.randint(0, 3, (M, C, side, side), generator=gen).double())
    s = torch.tensor(MBSTD_SIGNS[G], dtype=torch.float64)
    x = (a.unsqueeze(0) + s.view(G, 1, 1, 1, 1) * d.unsqueeze(0)).reshape(N, C, side, side)
    dy = qint(gen, (N, C + F, side, side))
    unit = c * HW * G
    T = None
    if unit & (unit - 1) == 0:
        T = qint(gen, (M, F))
        extra = dy[:, C:].reshape(G, M, F, HW).clone()             # sample g M + m
        rest = extra.sum((0, 3)) - extra[G - 1, :, :, HW - 1]
        extra[G - 1, :, :, HW - 1] = T * unit - rest
        dy[:, C:] = extra.reshape(N, F, side, side)
        assert torch.equal(dy[:, C:].reshape(G, M, F, HW).sum((0, 3)), T * unit)
    return dict(x=x, dy=dy, a=a, d=d, s=s, T=T, side=side)


def mbstd_exact_expect(shape, case):
    """exact mode, in closed form: the statistic is the mean of d over the group's c HW positions and dx = dy[:, :C] + T[m, f] s[g]"""
    N, C, HW, G, F = shape
    M, c = N // G, C // F
    stat = case["d"].reshape(M, F, c * HW).mean(-1)                                                 # [M, F]
    y = torch.cat([case["x"], stat.view(1, M, F, 1, 1).expand(G, M, F, case["side"], case["side"]).reshape(N, F, case["side"], case["side"])], 1)
    k = case["T"].view(1, M, F, 1, 1, 1) * case["s"].view(G, 1, 1, 1, 1, 1)
    dx = case["dy"][:, :C] + k.expand(G, M, F, c, case["side"], case["side"]).reshape(N, C, case["side"], case["side"])
    return y, dx


def mbstd_composite64(x, G, F, dy=None):
    """the layer as the reference composes it, float64 -> y (and dx for dy)"""
    N, C, H, W = x.shape
    xr = x.clone().requires_grad_(True)
    y = xr.reshape(G, -1, F, C // F, H, W)
    y = y - y.mean(dim=0)
    y = (y.square().mean(dim=0) + 1e-8).sqrt().mean(dim=[2, 3, 4]).reshape(-1, F, 1, 1).repeat(G, 1, H, W)
    y = torch.cat([xr, y], dim=1)
    if dy is None:
        return y.detach()
    return y.detach(), torch.autograd.grad(y, xr, dy)[0]


# ---------------------------------------------------------------------------------------------------------------- grouped GEMM

def gg_problem(gen, m, n, k0, k1=None, a_form="row", b_form="row", bias=False, rowsum=False, strided_c=False, alpha=(0.5, -2.0)):
    """one problem of a table, float64: a_t [m, k_t], b_t [k_t, n] small integers, alphas / scales powers of two.  a_form 'row' (unit column
    stride) / 'col' (unit row stride: the transpose of a [k, m] tensor); b_form 'row' ([k, n], unit column stride) / 'col' (the transpose of
    an [n, k] tensor, unit row stride).  -> dict with the operands, the forms and the references c, rowsum (None when not asked for)"""
    ks = [k0] + ([k1] if k1 is not None else [])
    terms = [(qint(gen, (m, k)), qint(gen, (k, n)), al) for k, al in zip(ks, alpha)]
    c = sum(al * (a @ b) for a, b, al in terms)
    pr = dict(m=m, n=n, terms=terms, a_form=a_form, b_form=b_form, strided_c=strided_c, bias=None, rowsum=None)
    if bias:
        pr["bias"], pr["bias_scale"] = qint(gen, (n,)), 0.5
        c = c + 0.5 * pr["bias"]
    if rowsum:
        pr["rowsum_scale"] = 2.0
        pr["rowsum"] = 2.0 * terms[0][0].sum(1)
    pr["c"] = c
    # range of every partial sum: products of magnitude <= 4, |alpha| <= 2, half-integer bias
    pr["bound"] = 2.0 * 4.0 * sum(ks) + 1.0
    return pr


GG_TABLES = [(16, None), (17, None), (33, None), (17, 8)]          # (problems, index of the M = 0 problem); one launch takes 16 non-empty ones
GG_LAUNCHES = {(16, None): [16], (17, None): [16, 1], (33, None): [16, 16, 1], (17, 8): [16]}


def gg_table(count, empty_at=None, seed=0):
    """a table of `count` problems: M, N on both sides of the 64-wide tile and K on both sides of the 16-deep step, all four stride forms,
    a second term with K1 != K0, bias, row sums (N > 64 among them: only the first column tile writes them), K0 = 0 with and without a bias,
    a strided c, and with `empty_at` one problem with M = 0 at that index"""
    gen = torch.Generator().manual_seed(700 + seed)
    sizes = [(m, n, k) for m in (63, 64, 65) for n in (63, 64, 65) for k in (15, 16, 17)]
    table = []
    for i in range(count):
        m, n, k = sizes[(i * 7 + seed) % len(sizes)]                         # 7 is coprime to 27: a table of 27 or more holds every triple
        kw = dict(a_form=("row", "col")[i % 2], b_form=("row", "col")[(i // 2) % 2], bias=i % 3 == 0, rowsum=i % 4 == 1, strided_c=i % 5 == 2)
        if i % 6 == 3:
            kw["k1"] = (33, 1, 16)[(i // 6) % 3]
        if i == 4:
            k = 0                                                            # zeros
        if i == 9:
            k, kw["bias"] = 0, True                                          # the bias alone
        if i == empty_at:
            m = 0                                                            # writes nothing
        if i == 5:
            n, kw["rowsum"] = 130, True                                      # three column tiles, one of them writes the row sums
        table.append(gg_problem(gen, m, n, k, **kw))
    return table
