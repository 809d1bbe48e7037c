"""What the Linear GEMM kernels (csrc/sn_gemm.hip) are held to, shared by tests/test_linear_truth.py (CPU) and
tests/test_linear_forms_gpu.py: seeded operands, one float64 reference per entry point written from the formulas in
include/sn_spmm.h with plain torch expressions (nothing from `kernels`), the per-element bound, and a numpy model of the
two-piece fp16 product with a switch that loses one correction product.  Imports no GPU code; every function takes the device.

THE BOUND, per output element.  S = |a|·|w| is the float64 product of absolute values and `scale` the sum of the absolute
values of every term of the entry point's formula (forward: S + |bias or segbias| + |residual|; input gradient through the
activation: (S + |x - center||B| + |Cc| + |rowmask·segvec|)·|elu'| + |gadd|).  Then

    tol = (4·sqrt(contraction) + 8) · 2^-24 · scale

4·sqrt(K)·2^-24 is the project's own bound of these kernels against float64 (tests/test_dense_gpu.py, the row-and-column
scaling test); the 8 is one fp32 rounding for each operation of the longest epilogue (subtract centre, times B, plus Cc, plus
per-mesh vector, plus product, form e + 1, times derivative, plus gadd), each at most 2^-24 of a partial result that `scale`
bounds.  The activated copy: tol + 1.2e-7 + 2^-24 — ELU is 1-Lipschitz, 1.2e-7 is the absolute error sn_gemm.hip states for its
__expf(x) - 1 form (above elu1).  Nothing here is fitted to what the kernels return."""
import zlib

import numpy as np
import torch

EPS = 2.0 ** -24
ELU_ABS = 1.2e-7 + EPS
PLANTED = (0.0, -0.0, -1.0, float(np.nextafter(np.float32(-1.0), np.float32(0.0))))      # legal ELU outputs at the derivative's edges


# ---- operands --------------------------------------------------------------------------------------------------------------
def _randn(shape, device, *key):
    g = torch.Generator(device=device)
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return torch.randn(shape, generator=g, device=device, dtype=torch.float32)


def row_factors(rows, device):
    """2^((r mod 41) - 20): one power of two per data row (no spread inside a row: the kernel documents a loss beyond 2^28
    inside one row)."""
    return torch.exp2(((torch.arange(rows, device=device) % 41) - 20).to(torch.float32))


def col_factors(n, device):
    """2^((c mod 21) - 10): one power of two per weight column — the unit the kernel scales."""
    return torch.exp2(((torch.arange(n, device=device) % 21) - 10).to(torch.float32))


def _check_flavour(flavour):
    if flavour not in ("plain", "magnitudes"):
        raise KeyError(flavour)


def fwd_operands(rows, K, J, flavour, device):
    """x (rows, K), W (J, K), bias (J), residual (rows, J).  magnitudes: rows of x and rows of W (the forward's weight
    columns: one per output) times powers of two."""
    _check_flavour(flavour)
    key = (rows, K, J)
    x = _randn((rows, K), device, "x", *key)
    W = _randn((J, K), device, "W", *key) / float(np.sqrt(K))
    if flavour == "magnitudes":
        x *= row_factors(rows, device)[:, None]
        W *= col_factors(J, device)[:, None]
    return dict(x=x, W=W, bias=_randn((J,), device, "bias", *key), residual=_randn((rows, J), device, "res", *key))


def elu_output(rows, C, device, *key):
    """elu(randn) in fp32 — every value a legal ELU output — with 0.0, -0.0, -1.0 and nextafter(-1, 0) planted in the first row
    (columns 0 .. 3) and in the last row (columns C/2 - 4 .. C/2 - 1: still in the half that goes through the activation)."""
    u = _randn((rows, C), device, "u", *key)
    x = torch.where(u > 0, u, torch.expm1(u))
    p = torch.tensor(PLANTED, dtype=torch.float32, device=device)
    x[0, 0:4] = p
    x[rows - 1, C // 2 - 4:C // 2] = p
    return x


def dgrad_operands(rows, C, J, flavour, device):
    """dy (rows, J), W (J, C), x (rows, C) = elu_output, center / B / Cc (C), gadd (rows, C).  magnitudes: rows of dy and
    columns of W (the input gradient's weight columns: one per output) times powers of two."""
    _check_flavour(flavour)
    key = (rows, C, J)
    dy = _randn((rows, J), device, "dy", *key)
    W = _randn((J, C), device, "Wd", *key) / float(np.sqrt(J))
    if flavour == "magnitudes":
        dy *= row_factors(rows, device)[:, None]
        W *= col_factors(C, device)[None, :]
    return dict(dy=dy, W=W, x=elu_output(rows, C, device, *key), center=_randn((C,), device, "center", *key),
                B=_randn((C,), device, "B", *key), Cc=_randn((C,), device, "Cc", *key), gadd=_randn((rows, C), device, "gadd", *key))


def seg_vectors(nseg, width, device, *key):
    return _randn((nseg, width), device, "seg", nseg, width, *key)


def row_mask(rows, device):
    """0 / 1 per row, every fifth row masked out."""
    return (torch.arange(rows, device=device) % 5 != 0).to(torch.float32)


def uniform_meshes(rows):
    """(nseg, rows_per_seg) for the uniform per-mesh forms: the factorisation of `rows` with the fewest meshes — more than one
    where the row count allows it — of at least 32 rows each; a row count without such a factorisation is one mesh."""
    for nseg in range(2, rows // 32 + 1):
        if rows % nseg == 0:
            return nseg, rows // nseg
    return 1, rows


def ragged_lengths(rows):
    """Mesh lengths for the ragged forms: each at least 32, not all multiples of 32, summing to `rows`."""
    head = [45, 32, 700, 33]
    rest = rows - sum(head)
    if rest < 64:
        return [rows]
    a = rest // 3 + 1
    return head + [a, rest - a]


def mesh_of_rows(rows, device, rows_per_seg=None, lengths=None):
    """mesh(r) as the header defines it: r / rows_per_seg, or the ragged mesh whose row range holds r."""
    if lengths is not None:
        return torch.repeat_interleave(torch.arange(len(lengths), device=device), torch.as_tensor(lengths, device=device))
    return torch.arange(rows, device=device) // rows_per_seg


# ---- float64 references (include/sn_spmm.h), each with its `scale` ------------------------------------------------------------
def elu64(v):
    return torch.where(v > 0, v, torch.expm1(v))


def elu_prime_of_output(o):
    """elu'(u) from o = elu(u): 1 for o > 0, o + 1 otherwise."""
    return torch.where(o > 0, torch.ones_like(o), o + 1)


def ref_fwd(x, W, bias=None, residual=None, segbias=None, mesh=None):
    """y[r, j] = sum_k x[r, k] W[j, k] + bias[j] | segbias[mesh(r), j] (+ residual[r, j]).  -> (y, scale), float64."""
    xd, Wd = x.double(), W.double()
    y = xd @ Wd.t()
    scale = xd.abs() @ Wd.abs().t()
    b = segbias.double()[mesh] if segbias is not None else bias.double()
    y += b
    scale += b.abs()
    if residual is not None:
        y += residual.double()
        scale += residual.double().abs()
    return y, scale


def ref_dgrad(dy, W, x=None, center=None, B=None, Cc=None):
    """dx[r, c] = sum_j dy[r, j] W[j, c] (+ (x[r, c] - center[c]) B[c] + Cc[c] when B is given).  -> (dx, scale), float64."""
    dyd, Wd = dy.double(), W.double()
    dx = dyd @ Wd
    scale = dyd.abs() @ Wd.abs()
    if B is not None:
        xc = x.double() - center.double() if center is not None else x.double()
        dx += xc * B.double() + Cc.double()
        scale += xc.abs() * B.double().abs() + Cc.double().abs()
    return dx, scale


def ref_dgrad_act(dy, W, x, center, B, Cc, segvec=None, mesh=None, rowmask=None, gadd=None):
    """gact[r, c] = (dy[r]·W[:, c] + (x[r, c] - center[c]) B[c] + Cc[c] + rowmask[r] segvec[mesh(r), c]) elu'(x[r, c]) + gadd[r, c]
    for every column handed in (slice the column operands for half of them).  -> (gact, scale), float64."""
    g, scale = ref_dgrad(dy, W, x, center, B, Cc)
    if segvec is not None:
        sv = segvec.double()[mesh]
        if rowmask is not None:
            sv = sv * rowmask.double()[:, None]
        g += sv
        scale += sv.abs()
    d = elu_prime_of_output(x.double())
    g *= d
    scale *= d.abs()
    if gadd is not None:
        g += gadd.double()
        scale += gadd.double().abs()
    return g, scale


# ---- the bound -----------------------------------------------------------------------------------------------------------------
def tol_of(scale, contraction):
    return (4.0 * float(np.sqrt(contraction)) + 8.0) * EPS * scale


def tol_elu_of(scale, contraction):
    return tol_of(scale, contraction) + ELU_ABS


def worst_ratio(got, ref, tol, scale):
    """max err / tol over the outputs (inf for a non-finite output where `scale` is finite and below 1e38, and for an error
    where the bound is zero); the comparison itself is elementwise, |got - ref| <= tol, on the tensors' own device."""
    got = got.double()
    must = torch.isfinite(scale) & (scale < 1e38)
    if not bool(torch.isfinite(got[must]).all()):
        return float("inf")
    err = (got - ref).abs()[must]
    t = tol[must] if torch.is_tensor(tol) else torch.full_like(err, tol)
    if not bool((err <= t).all()):
        bad = err > t
        return float((err[bad] / t[bad]).max()) if bool((t[bad] > 0).all()) else float("inf")
    pos = t > 0
    return float((err[pos] / t[pos]).max()) if bool(pos.any()) else 0.0


# ---- numpy model of the two-piece product (sn_gemm.hip, "EXACT two-piece split") ------------------------------------------------
def pow2_up(m):
    """2^(14 - E) for an absolute maximum m = f·2^E, f in [0.5, 1) (exponent clamped to +-100 as in pow2_scales)."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    e = ((m.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64) - 126
    return np.exp2(14 - np.clip(e, -100, 100)).astype(np.float32)


def _pieces(a):
    """H = rn16(a), L = rn16((a - H)·2^11) of an already scaled fp32 array, both back in fp32."""
    f32, f16 = np.float32, np.float16
    H = a.astype(f16).astype(f32)
    L = ((a - H) * f32(2048)).astype(f16).astype(f32)
    return H, L


def split_model(x, W, drop=()):
    """y = x·W^T (x: rows x K, W: J x K; no epilogue) as gemm_rows_split_k forms it: every row of x and every row of W scaled by
    2^(14 - E) of its own absolute maximum, H = rn16(a·up), L = rn16((a·up - H)·2^11), the three partial products hh, hl (x high,
    W low) and lh (x low, W high) accumulated in fp32 — 16 exact products per step, as the matrix instruction takes them — then
    hh + 2^-11 (hl + lh) and the exact inverse scales.  drop: names of partial products ("hl", "lh") a faulty kernel loses."""
    f32, f64 = np.float32, np.float64
    x, W = np.asarray(x, f32), np.asarray(W, f32)
    rup, cup = pow2_up(np.abs(x).max(1)), pow2_up(np.abs(W).max(1))
    xh, xl = _pieces(x * rup[:, None])
    wh, wl = _pieces(W * cup[:, None])
    K = x.shape[1]
    acc = {}
    for name, a, b in (("hh", xh, wh), ("hl", xh, wl), ("lh", xl, wh)):
        s = np.zeros((x.shape[0], W.shape[0]), f32)
        if name not in drop:
            for k in range(0, K, 16):
                s = (s.astype(f64) + a[:, k:k + 16].astype(f64) @ b[:, k:k + 16].astype(f64).T).astype(f32)
        acc[name] = s
    y = ((acc["hl"] + acc["lh"]).astype(f64) * 2.0 ** -11 + acc["hh"].astype(f64)).astype(f32)      # one fused multiply-add
    return y * (f32(1) / rup)[:, None] * (f32(1) / cup)[None, :]
