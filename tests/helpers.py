"""Shared test helpers: seeded meshes/operators and comparison utilities."""
import os

import numpy as np
import scipy.sparse as sp

from surfacenetworks_amd import mesh_ops


def load_golden(golden_dir, name):
    """The arrays of the fixture tests/golden/<name>: the file itself or, for a fixture written in parts to keep every file
    under 1 MiB (make_golden.save), <stem>_part0.npz, <stem>_part1.npz, ... merged in order."""
    path = os.path.join(golden_dir, name)
    if os.path.exists(path):
        return np.load(path, allow_pickle=False)
    out, i = {}, 0
    while os.path.exists(part := os.path.join(golden_dir, f"{name[:-len('.npz')]}_part{i}.npz")):
        with np.load(part, allow_pickle=False) as z:
            out.update((k, z[k]) for k in z.files)
        i += 1
    if not i:
        raise FileNotFoundError(path)
    return out


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def mesh_fixture(kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "cloth":
        V, F = mesh_ops.grid_cloth(13, 9, rng)
    elif kind == "cloth_perm":
        V, F = mesh_ops.grid_cloth(11, 10, rng, permute=True)
    elif kind == "torus":
        V, F = mesh_ops.torus_grid(9, 12, rng)
    elif kind == "delaunay":
        V, F = mesh_ops.delaunay_disc(150, rng)
    else:
        raise KeyError(kind)
    return V, F, mesh_ops.mesh_operators(V, F)


def random_csr(M, K, density, seed, empty_rows=()):
    A = sp.random(M, K, density=density, format="lil", dtype=np.float32, random_state=seed)
    for r in empty_rows:
        A.rows[r] = []
        A.data[r] = []
    A = A.tocsr()
    A.sort_indices()
    return A


# ---- the Linear kernels address their operands through raw buffer windows (sn_gemm.hip RowWindow, wgrad16_k): tests place
# every operand as a strided view inside an arena of NaNs, every output as a view inside an arena of canaries ---------------
def _arena(rows, width, pad_rows=3, pad_cols=8, seed=0, fill=float("nan"), device="cuda", values=None):
    """(arena, view): `view` = rows x width of random values (or of `values`, a rows x width tensor) inside a poisoned arena
    (rows before / after, columns on both sides; the view's leading dimension is width + 2·pad_cols, 16-byte aligned)."""
    import torch

    a = torch.full((rows + 2 * pad_rows, width + 2 * pad_cols), fill, device=device)
    v = a[pad_rows:pad_rows + rows, pad_cols:pad_cols + width]
    if values is None:
        values = torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, width)).astype(np.float32))
    v.copy_(values)
    return a, v


def _outside_untouched(arena, view_rows, width, canary, pad_rows=3, pad_cols=8):
    import torch

    m = torch.ones_like(arena, dtype=torch.bool)
    m[pad_rows:pad_rows + view_rows, pad_cols:pad_cols + width] = False
    return bool((arena[m] == canary).all())


# ---- deterministic, library-independent parameter fill (golden fixtures store no weights) ------------------
def _splitmix_uniform(n, seed):
    """n doubles in [0,1) from splitmix64 on (index, seed): exact integer arithmetic, identical everywhere."""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15) % (1 << 64))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def det_tensor(shape, seed, scale=1.0):
    n = int(np.prod(shape)) if len(shape) else 1
    return ((_splitmix_uniform(n, seed) - 0.5) * 2 * scale).astype(np.float32).reshape(shape)


def deterministic_init(module, seed=0):
    """Fill every parameter/buffer of a torch module from splitmix64, keyed by its position in state_dict()."""
    import torch

    sd = module.state_dict()
    new = {}
    for i, (k, v) in enumerate(sd.items()):
        if k.endswith("num_batches_tracked"):
            new[k] = torch.zeros_like(v)
        elif k.endswith("running_var"):
            new[k] = torch.from_numpy(1.0 + 0.5 * det_tensor(tuple(v.shape), seed * 1000 + i, 1.0))
        elif k.endswith("bn.weight"):
            new[k] = torch.from_numpy(1.0 + 0.3 * det_tensor(tuple(v.shape), seed * 1000 + i, 1.0))
        else:
            fan_in = v.shape[1] if v.dim() == 2 else 8
            new[k] = torch.from_numpy(det_tensor(tuple(v.shape), seed * 1000 + i, 1.0 / np.sqrt(fan_in)))
    module.load_state_dict(new)
    return module


def grad_signature(module):
    """Per-parameter [L2 norm, sum, first 4 entries] of .grad — a compact stand-in for the full gradient."""
    out = {}
    for k, p in module.named_parameters():
        g = p.grad.detach().double().cpu().reshape(-1)
        head = np.zeros(4)
        head[: min(4, g.numel())] = g[:4].numpy()
        out[k] = np.concatenate([[float(g.norm()), float(g.sum())], head])
    return out


def sigs_close(sigs, ref_of, tol=1e-4):
    """Gradient signatures agree when every entry is within tol * (L2 norm of that gradient) + 1e-5 * (largest
    gradient norm in the model).  The floor matters for parameters whose exact gradient is zero (a Linear bias that
    feeds a BatchNorm): their computed gradient is pure round-off.  Returns the list of offending keys."""
    top = max(abs(float(ref_of(k)[0])) for k in sigs)
    bad = []
    for k, s in sigs.items():
        r = np.asarray(ref_of(k))
        if not (np.abs(np.asarray(s) - r) <= tol * abs(r[0]) + 1e-5 * top).all():
            bad.append((k, s, r))
    return bad


# ---- the two-piece fp16 weight gradient (wgrad16_k<CT, WgradHalf2>, csrc/sn_dense.hip): a numpy model of its split and probe operands ----------
def pow2_up_for(bound):
    """The power of two wgrad16_k<CT, WgradHalf2> scales an operand by: bound = f * 2^E, f in [0.5, 1)  ->  2^(15 - E), which brings the bound
    into [2^14, 2^15) (the exponent is clamped to +-100 for zero / denormal / non-finite bounds, as in the kernel)."""
    b = np.ascontiguousarray(bound, dtype=np.float32)
    e = ((b.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64) - 126
    return np.exp2(15 - np.clip(e, -100, 100)).astype(np.float32)


def wgrad_xbound(xinvstd, stat_rows):
    """The bound of |x - center| per column that the kernel really scales by: sqrtf(stat_rows) * 1.0625f / xinvstd[c] in fp32
    (make_bounds; the factor covers the rounding of the statistics)."""
    xfac = np.float32(np.sqrt(np.float32(stat_rows))) * np.float32(1.0625)
    return (xfac / np.asarray(xinvstd, dtype=np.float32)).astype(np.float32)


def wgrad_split_model(dy, x, center, dybound, xinvstd, stat_rows, drop=()):
    """G = dy^T (x - center) as the two-piece kernel forms it: operands scaled by pow2_up_for of their bounds, a = h + l with
    h = fp16(a), l = fp16(a - h), the products l*h, h*l, h*h (never l*l) accumulated in fp32 row by row, exact inverse scales.
    `drop` names products to leave out ("hh", "hl", "lh": dy piece first) and "ll" may be ADDED with drop=("-ll",)."""
    f32, f16 = np.float32, np.float16
    sdy = pow2_up_for(f32(np.max(dybound)))
    sx = pow2_up_for(wgrad_xbound(xinvstd, stat_rows))
    a = np.asarray(dy, f32) * sdy
    b = np.clip((np.asarray(x, f32) - np.asarray(center, f32)[None, :]) * sx[None, :], f32(-65504), f32(65504))
    ah, bh = a.astype(f16).astype(f32), b.astype(f16).astype(f32)
    al, bl = (a - ah).astype(f16).astype(f32), (b - bh).astype(f16).astype(f32)
    acc = np.zeros((a.shape[1], b.shape[1]), f32)
    terms = [("lh", al, bh), ("hl", ah, bl), ("hh", ah, bh)] + ([("ll", al, bl)] if "-ll" in drop else [])
    for r in np.flatnonzero(np.any(a != 0, axis=1) & np.any(b != 0, axis=1)):
        for name, p, q in terms:
            if name not in drop:
                acc = acc + np.outer(p[r], q[r]).astype(f32)
    return acc * ((f32(1) / sx) * (f32(1) / sdy))[None, :]


_PROBE_PATTERNS = ((1.0, 1), (1.0 + 2.0 ** -10, 11), (1.0 + 2.0 ** -21, 22), (1.5, 2))      # (mantissa, significant bits)


def _probe_row(n, unit, seed):
    """n elements unit[i] * 2^-k * u: k = i % 40, u cycling through _PROBE_PATTERNS every 40 elements (k = 0: u = 1, the
    element then sits AT the power of two below its bound), alternating signs.  -> values (fp64), k, significant bits."""
    i = np.arange(n)
    k = i % 40
    pat = (i // 40 + seed) % len(_PROBE_PATTERNS)
    u = np.array([p[0] for p in _PROBE_PATTERNS])[pat]
    bits = np.array([p[1] for p in _PROBE_PATTERNS])[pat]
    u = np.where(k == 0, 1.0, u)
    bits = np.where(k == 0, 1, bits)
    return np.where(i % 2 == 0, 1.0, -1.0) * unit * np.exp2(-k.astype(np.float64)) * u, k, bits


def split_probe_operands(J, C, rows, nz_row, seed=0):
    """Operands that probe the split of wgrad16_k<CT, WgradHalf2> element by element: dy and x are zero except in row `nz_row`, so
    G[j, c] = dy[j] * x[c] is ONE product per output (nothing for the fp32 accumulation to round but the pieces of that term).
    dy[j] = unit_dy * 2^-k_j * u_j and x[c] = unit_c * 2^-m_c * w_c, unit = the power of two at or below the operand's bound
    (what the kernel's scale maps to 2^14).  Returns a dict with the operands, the bounds and, per pair (j, c):
      exact   k, m <= 17, one factor of <= 11 bits (its low piece is zero: the dropped l*l product is absent) and a product
              of <= 24 bits (the fp32 accumulator holds it): the kernel must reproduce float64 exactly;
      loose_dy / loose_x   that operand 17 < k <= 39 below its bound, the other a power of two with k <= 17: the header's
              absolute error, 2^-39 of the bound times the other operand."""
    rng = np.random.default_rng(seed)
    bound = np.float32(1.75 * 2.0 ** int(rng.integers(-6, 7)))
    xinvstd = (np.exp2(rng.integers(-8, 9, size=C)) * rng.uniform(1.0, 2.0, size=C)).astype(np.float32)
    stat_rows = max(rows, 1000)
    xb = wgrad_xbound(xinvstd, stat_rows)
    unit_dy = 2.0 ** 14 / float(pow2_up_for(bound).reshape(-1)[0])
    unit_x = 2.0 ** 14 / pow2_up_for(xb).astype(np.float64)
    dyr, k, kb = _probe_row(J, unit_dy, seed)
    xr, m, mb = _probe_row(C, unit_x, seed + 1)
    dy = np.zeros((rows, J), np.float32)
    x = np.zeros((rows, C), np.float32)
    dy[nz_row] = dyr.astype(np.float32)
    x[nz_row] = xr.astype(np.float32)
    assert np.array_equal(dy[nz_row].astype(np.float64), dyr) and np.array_equal(x[nz_row].astype(np.float64), xr)
    assert np.abs(dy).max() <= bound and (np.abs(x).max(0) <= xb).all()          # the bounds handed over are true
    K, M, KB, MB = k[:, None], m[None, :], kb[:, None], mb[None, :]
    return dict(dy=dy, x=x, center=np.zeros(C, np.float32), bound=bound, xinvstd=xinvstd, stat_rows=stat_rows, xbound=xb,
                ref=np.outer(dyr, xr), dy_row=dyr, x_row=xr, k=k, m=m, kbits=kb, mbits=mb,
                exact=(K <= 17) & (M <= 17) & (np.minimum(KB, MB) <= 11) & (KB + MB <= 24),
                loose_dy=(K > 17) & (M <= 17) & (MB == 1), loose_x=(M > 17) & (K <= 17) & (KB == 1))


def top_of_binade_operands(J, C, rows, nz_row):
    """One non-zero row whose dy elements ARE the bound and whose bound sits at the top of its binade (mantissa all ones:
    scaled by pow2_up_for it lands just below 2^15, the largest scaled value the contract allows — one more binary order would
    pass fp16's 65504), times powers of two in x; and in the even columns of x an element equal to the column's own bound,
    itself chosen within 2^-12 of a power of two."""
    bound = np.nextafter(np.float32(8.0), np.float32(0))
    stat_rows = max(rows, 1000)
    xfac = np.float32(np.sqrt(np.float32(stat_rows))) * np.float32(1.0625)
    target = (np.exp2(np.arange(C) % 9 - 4) * (1 - 2.0 ** -13)).astype(np.float32)
    xinvstd = (xfac / target).astype(np.float32)
    xb = wgrad_xbound(xinvstd, stat_rows)
    assert (np.frexp(xb)[0] > 65520.0 / 65536.0).all() and float(np.frexp(bound)[0]) > 65520.0 / 65536.0
    unit_x = 2.0 ** 14 / pow2_up_for(xb).astype(np.float64)
    j, c = np.arange(J), np.arange(C)
    dyr = np.where(j % 2 == 0, 1.0, -1.0) * float(bound) * np.exp2(-(j % 8).astype(np.float64))
    xr = np.where(c % 2 == 0, xb.astype(np.float64), unit_x * np.exp2(-(c % 8).astype(np.float64)))
    dy = np.zeros((rows, J), np.float32)
    x = np.zeros((rows, C), np.float32)
    dy[nz_row], x[nz_row] = dyr.astype(np.float32), xr.astype(np.float32)
    assert np.array_equal(dy[nz_row].astype(np.float64), dyr) and np.array_equal(x[nz_row].astype(np.float64), xr)
    return dict(dy=dy, x=x, center=np.zeros(C, np.float32), bound=bound, xinvstd=xinvstd, stat_rows=stat_rows, xbound=xb,
                ref=np.outer(dyr, xr), pow2_x=(c % 2 == 1))
