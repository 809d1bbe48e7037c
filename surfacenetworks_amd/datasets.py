"""Readers for the reference's on-disk dataset formats -> device-resident pools.

The reference stores its preprocessed data as pickled numpy object arrays:

  ARAP        as_rigid_as_possible/data_plus/<seq>.npy  : list of 50 frame dicts {'V' (nV,3) f32, 'F' (nF,3) i32} with
              {'L','Di','DiA'} scipy CSR float32 on the first 10 frames
              (written by src/as_rigid_as_possible/add_laplacian.py:61-70, read by main.py:58-94)
  Mesh-MNIST  mesh_mnist/data/{train,test}_plus.np       : list of dicts {'V','F','L','flat_L','Di','DiA','flat_Di',
              'flat_DiA','label'}  (src/mesh_mnist/add_laplacian.py:63-71, read by main.py:54-72)
  FAUST       *.npz with V, F, L, D, DA (0-d object arrays holding scipy matrices), label, label_inv, dist_mat
              (read by src/dense_correspondence/main.py:65-104)

Loading them needs `allow_pickle=True` (they ARE pickles); only load files you trust.  The writers below produce the
same layouts from synthetic meshes so that the readers are testable without the (undownloadable) datasets.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from . import arap as _arap
from . import mesh_ops
from .operators import OperatorPool

__all__ = ["load_arap_sequence", "arap_from_files", "load_mesh_mnist", "mnist_from_samples", "mesh_mnist_from_images", "mesh_digit_samples", "load_faust_frame", "faust_from_files", "faust_frame_from_mesh", "normal_frame_from_mesh",
           "write_arap_sequence", "write_mesh_mnist", "write_faust_frame"]


# ---- ARAP ---------------------------------------------------------------------------------------------------
def load_arap_sequence(path: str) -> List[Dict]:
    """One <seq>.npy as a list of frame dicts (numpy / scipy objects, untouched)."""
    seq = np.load(path, encoding="latin1", allow_pickle=True)          # as main.py:59
    return list(seq)


def arap_from_files(paths: Sequence[str], device="cuda", model="dir", reorder="auto") -> "_arap.ClothSequences":
    """Build the resident ARAP dataset (frame coordinates + operator pools) from reference sequence files.
    Returns an object with the ClothSequences interface (sample_batch, ...).
    reorder ("auto" / True / False): the sequences are STORED in a locality numbering of their vertices and faces
    (mesh_ops.MeshOrder; the files keep whatever order the scanner / simulator wrote): coordinates are permuted once, the
    stored operators become P_r A P_c^T; `ds.to_dataset_order(outputs, seq_ids)` maps per-vertex results back."""
    seqs = [load_arap_sequence(p) for p in paths]
    ds = _arap.ClothSequences.__new__(_arap.ClothSequences)
    ds.device = torch.device(device)
    ds.kind, ds.operators = model, "pool"
    ds.n = len(seqs)
    ds.frames = min(len(s) for s in seqs)
    ds.op_frames = min(sum(1 for fr in s if fr.get("Di" if model == "dir" else "L") is not None) for s in seqs)
    ds.num_vertices = np.array([s[0]["V"].shape[0] for s in seqs])
    ds.num_faces = np.array([s[0]["F"].shape[0] for s in seqs])
    ds.orders = [mesh_ops.MeshOrder.of_mesh(np.asarray(s[0]["F"]), s[0]["V"].shape[0], reorder) for s in seqs]
    vmax = int(ds.num_vertices.max())
    xyz = np.zeros((ds.n, ds.frames, vmax, 3), np.float32)
    for i, s in enumerate(seqs):
        for t in range(ds.frames):
            xyz[i, t, : s[t]["V"].shape[0]] = ds.orders[i].vertex_rows(np.asarray(s[t]["V"], dtype=np.float32))
    ds.xyz = torch.from_numpy(xyz).to(ds.device)
    ds.vcount = torch.from_numpy(ds.num_vertices).to(ds.device)

    def pick(key, rows, cols, group):
        out = []
        for s, o in zip(seqs, ds.orders):
            for t in range(ds.op_frames):
                A = s[t][key].astype(np.float32)
                out.append(A if o.identity else mesh_ops.permute_operator(A, getattr(o, rows), getattr(o, cols), group))
        return out
    if model == "dir":
        ds.pool_Di = OperatorPool(pick("Di", "forder", "vorder", 4), ds.device, want_bsr4=True)
        ds.pool_DiA = OperatorPool(pick("DiA", "vorder", "forder", 4), ds.device, want_bsr4=True)
    else:
        ds.pool_L = OperatorPool(pick("L", "vorder", "vorder", 1), ds.device)
    return ds


def write_arap_sequence(path: str, Vt: np.ndarray, F: np.ndarray, op_frames: int = 10) -> None:
    """Write a sequence in the reference layout (add_laplacian.py:45-70): operators on the first `op_frames` frames."""
    frames = []
    for t in range(Vt.shape[0]):
        fr = {"V": Vt[t].astype("float32"), "F": F.astype("int32")}
        if t < op_frames:
            ops = mesh_ops.mesh_operators(Vt[t].astype(np.float64), F)
            fr.update({"L": ops["L"], "Di": ops["Di"], "DiA": ops["DiA"]})
        frames.append(fr)
    arr = np.empty(len(frames), dtype=object)
    arr[:] = frames
    with open(path, "wb") as fh:
        np.save(fh, arr, allow_pickle=True)


# ---- Mesh-MNIST --------------------------------------------------------------------------------------------------
def load_mesh_mnist(path: str) -> List[Dict]:
    with open(path, "rb") as fh:                                        # as main.py:54
        return list(np.load(fh, encoding="latin1", allow_pickle=True))


def mnist_from_samples(samples: Sequence[Dict], device="cuda", model="dir", reorder="auto"):
    """Resident Mesh-MNIST dataset (MeshDigits interface) from reference sample dicts; `reorder`: stored in a locality numbering
    (mesh_ops.MeshOrder — the file's operators become P_r A P_c^T; the model's output is per mesh, nothing maps back)."""
    from . import mesh_mnist as mm

    orders = [mesh_ops.MeshOrder.of_mesh(np.asarray(s["F"]), s["V"].shape[0], reorder) for s in samples]

    def op(i, key, rows, cols, group):
        A, o = samples[i][key].astype(np.float32), orders[i]
        return A if o.identity else mesh_ops.permute_operator(A, getattr(o, rows), getattr(o, cols), group)

    ds = mm.MeshDigits.__new__(mm.MeshDigits)
    ds.device, ds.kind, ds.n = torch.device(device), model, len(samples)
    ds.nv = np.array([s["V"].shape[0] for s in samples])
    ds.nf = np.array([s["F"].shape[0] for s in samples])
    xyz = np.zeros((ds.n, int(ds.nv.max()), 3), np.float32)
    for i, s in enumerate(samples):
        xyz[i, : ds.nv[i]] = orders[i].vertex_rows(np.asarray(s["V"], dtype=np.float32))
    ds.xyz = torch.from_numpy(xyz).to(ds.device)
    ds.vcount = torch.from_numpy(ds.nv).to(ds.device)
    ds.labels = torch.tensor([int(s["label"]) for s in samples], device=ds.device)
    if model == "dir":
        ds.pool_Di = OperatorPool([op(i, "Di", "forder", "vorder", 4) for i in range(ds.n)], ds.device, want_bsr4=True)
        ds.pool_DiA = OperatorPool([op(i, "DiA", "vorder", "forder", 4) for i in range(ds.n)], ds.device, want_bsr4=True)
    else:
        ds.pool_L = OperatorPool([op(i, "L", "vorder", "vorder", 1) for i in range(ds.n)], ds.device)
    ds.orders = orders
    ds.run_nv = ds.run_nf = 0
    return ds


_DIGITS_CHUNK = 4096      # images per launch of the maker (its padded outputs take 30 KiB per image)


def _digit_meshes(images, seed, r, device, min_points=101, min_det=None):
    """kernels.mesh_digits over `images`, _DIGITS_CHUNK at a time (image_base keeps the random stream keyed by the image's index
    in the whole array) -> (status, attempts, V list, F list): host arrays per image, V (n, 3) fp32 and F (nF, 3) int32 views
    cut to their sizes, empty for a rejected image."""
    from . import kernels

    img = images if torch.is_tensor(images) else torch.from_numpy(np.ascontiguousarray(images))
    if img.dim() != 3 or img.dtype != torch.uint8:
        raise ValueError(f"images must be (B, rows, cols) uint8, got {tuple(img.shape)} {img.dtype}")
    R = int(round(float(r) * mesh_ops.MESHDIGITS_Q))
    status, attempts, Vs, Fs = [], [], [], []
    for s in range(0, img.shape[0], _DIGITS_CHUNK):
        out = kernels.mesh_digits(img[s: s + _DIGITS_CHUNK].to(device), seed=seed, R=R, min_points=min_points, image_base=s,
                                  min_det=kernels.MESHDIGITS_MIN_DET if min_det is None else min_det)
        count, nF, V, F = (getattr(out, k).cpu().numpy() for k in ("count", "nF", "V", "F"))
        status.append(out.status.cpu().numpy())
        attempts.append(out.attempts.cpu().numpy())
        Vs += [V[b, : count[b]] for b in range(V.shape[0])]
        Fs += [F[b, : nF[b]] for b in range(F.shape[0])]
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int32)
    return cat(status), cat(attempts), Vs, Fs


def _warn_rejected(who, status):
    import warnings

    rejected = np.flatnonzero(status != 0)
    if rejected.size:
        warnings.warn(f"{who}: {rejected.size} image(s) found no mesh that passes the quality test in "
                      f"{mesh_ops.MESHDIGITS_MAX_ATTEMPTS} attempts and are left out: {rejected.tolist()}")
    return rejected


def _labels_for(who, labels, count):
    lab = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).reshape(-1)
    if lab.shape[0] != count:
        raise ValueError(f"{who}: {lab.shape[0]} labels for {count} images")
    return lab


def mesh_digit_samples(images, labels, seed=0, r=1.5, device="cuda") -> List[Dict]:
    """The reference's first Mesh-MNIST stage (src/mesh_mnist/create_data.py:62-105) on the device: a list of {'V' (n, 3) float32,
    'F' (nF, 3) int32, 'label'} dicts in create_data.py's own layout — unscaled pixel coordinates with the bilinear intensity as z
    — that the reference's add_laplacian.py or write_mesh_mnist take.  images: (B, rows, cols) uint8 (numpy or tensor).  Images
    that stay rejected after the retries are left out (warnings.warn names them)."""
    lab = _labels_for("mesh_digit_samples", labels, images.shape[0])
    status, _, Vs, Fs = _digit_meshes(images, seed, r, device)
    _warn_rejected("mesh_digit_samples", status)
    return [{"V": Vs[b].copy(), "F": Fs[b].copy(), "label": int(lab[b])} for b in range(len(Vs)) if status[b] == 0]


def _csr_block(A, r0, r1, c0, c1):
    """Rows r0..r1, columns c0..c1 of a block-diagonal scipy CSR whose rows r0..r1 have no entry outside those columns."""
    import scipy.sparse as sp

    ip = A.indptr[r0: r1 + 1]
    sl = slice(int(ip[0]), int(ip[-1]))
    return sp.csr_matrix((A.data[sl], A.indices[sl] - c0, ip - ip[0]), shape=(r1 - r0, c1 - c0))


def mesh_mnist_from_images(images, labels, seed=0, r=1.5, device="cuda", model="dir", reorder="auto", scale=True):
    """Images to a trainable Mesh-MNIST dataset on the device: the whole of src/mesh_mnist/create_data.py (Poisson-disc points,
    bilinear intensity, Delaunay, the area test with its retries: kernels.mesh_digits, one launch per 4096 images) and of
    add_laplacian.py (the operators, from the existing device builders on V / 27 - (0.5, 0.5, 0), add_laplacian.py:40-41).
    images: (B, rows, cols) uint8, 28 x 28 for MNIST; any size whose (cols - 1) x (rows - 1) pixel domain the sampler's grid takes
    (the divisor is then max(rows, cols) - 1).  labels: (B,).  r: the Poisson-disc radius in pixels.  scale=False keeps pixel
    coordinates.  Returns a dataset with the MeshDigits interface (pools, sample_batch, orders) for mesh_mnist.train_step and
    graphed_train_step.  Images that stay rejected after the retries are left out: `rejected` holds their indices (also named by
    a warnings.warn), `source` the image index of every mesh, `attempts` the attempt each mesh came from, `V` / `F` the stored
    (scaled, reordered) meshes as numpy arrays."""
    from . import mesh_mnist as mm
    from .operators import dirac_operators_from_mesh, laplacian_operator_from_mesh

    if model not in ("dir", "lap"):
        raise ValueError(f'mesh_mnist_from_images: model must be "dir" or "lap", got {model!r}')
    lab = _labels_for("mesh_mnist_from_images", labels, images.shape[0])
    status, attempts, Vs, Fs = _digit_meshes(images, seed, r, device)
    rejected = _warn_rejected("mesh_mnist_from_images", status)
    keep = np.flatnonzero(status == 0)
    if keep.size == 0:
        raise ValueError("mesh_mnist_from_images: no image gave a mesh")
    side = np.float32(max(images.shape[1], images.shape[2]) - 1)
    ds = mm.MeshDigits.__new__(mm.MeshDigits)
    ds.device, ds.kind, ds.n = torch.device(device), model, int(keep.size)
    ds.rejected, ds.source, ds.attempts = rejected, keep, attempts[keep]
    ds.orders, ds.V, ds.F = [], [], []
    for b in keep:
        Vb, Fb = Vs[b], Fs[b].astype(np.int64)
        if scale:                                   # fp32 division and subtraction, each rounded once
            Vb = Vb / side - np.array([0.5, 0.5, 0.0], np.float32)
        order = mesh_ops.MeshOrder.of_mesh(Fb, Vb.shape[0], reorder)
        Vb, Fb = order.mesh(Vb, Fb)
        ds.orders.append(order)
        ds.V.append(np.ascontiguousarray(Vb, dtype=np.float32))
        ds.F.append(np.ascontiguousarray(Fb, dtype=np.int32))
    ds.nv = np.array([v.shape[0] for v in ds.V])
    ds.nf = np.array([f.shape[0] for f in ds.F])
    # _DIGITS_CHUNK meshes at a time as ONE disjoint mesh: one run of the device builders, cut into per-mesh blocks for the pools
    mats = {"Di": [], "DiA": [], "L": []}
    for s in range(0, ds.n, _DIGITS_CHUNK):
        e = min(s + _DIGITS_CHUNK, ds.n)
        voff = np.concatenate([[0], np.cumsum(ds.nv[s:e])])
        foff = np.concatenate([[0], np.cumsum(ds.nf[s:e])])
        Vg = torch.from_numpy(np.concatenate(ds.V[s:e])).to(ds.device)
        Fg = torch.from_numpy(np.concatenate([f + np.int32(o) for f, o in zip(ds.F[s:e], voff[:-1])])).to(ds.device)
        if model == "dir":
            Di, DiA = (op.to_scipy() for op in dirac_operators_from_mesh(Vg, Fg))
            mats["Di"] += [_csr_block(Di, 4 * foff[i], 4 * foff[i + 1], 4 * voff[i], 4 * voff[i + 1]) for i in range(e - s)]
            mats["DiA"] += [_csr_block(DiA, 4 * voff[i], 4 * voff[i + 1], 4 * foff[i], 4 * foff[i + 1]) for i in range(e - s)]
        else:
            L = laplacian_operator_from_mesh(Vg, Fg).to_scipy()
            mats["L"] += [_csr_block(L, voff[i], voff[i + 1], voff[i], voff[i + 1]) for i in range(e - s)]
    if model == "dir":
        ds.pool_Di = OperatorPool(mats["Di"], ds.device, want_bsr4=True)
        ds.pool_DiA = OperatorPool(mats["DiA"], ds.device, want_bsr4=True)
    else:
        ds.pool_L = OperatorPool(mats["L"], ds.device)
    xyz = np.zeros((ds.n, int(ds.nv.max()), 3), np.float32)
    for i, v in enumerate(ds.V):
        xyz[i, : v.shape[0]] = v
    ds.xyz = torch.from_numpy(xyz).to(ds.device)
    ds.vcount = torch.from_numpy(ds.nv).to(ds.device)
    ds.labels = torch.from_numpy(lab[keep].astype(np.int64)).to(ds.device)
    ds.run_nv = ds.run_nf = 0
    return ds


def write_mesh_mnist(path: str, meshes: Sequence, labels: Sequence[int]) -> None:
    """meshes: iterable of (V, F).  Layout of add_laplacian.py:63-71 (flat_* variants included)."""
    out = []
    for (V, F), lab in zip(meshes, labels):
        ops = mesh_ops.mesh_operators(V, F)
        Vf = V.copy()
        Vf[:, 2] = 0
        flat = mesh_ops.mesh_operators(Vf, F)
        out.append({"V": V.astype("float32"), "F": F.astype("int32"), "L": ops["L"], "flat_L": flat["L"], "Di": ops["Di"],
                    "DiA": ops["DiA"], "flat_Di": flat["Di"], "flat_DiA": flat["DiA"], "label": int(lab)})
    arr = np.empty(len(out), dtype=object)
    arr[:] = out
    with open(path, "wb") as fh:
        np.save(fh, arr, allow_pickle=True)


# ---- FAUST ----------------------------------------------------------------------------------------------------------
def load_faust_frame(path: str, device="cuda") -> Dict:
    """One FAUST .npz as the frame dict of dense_correspondence/main.py:65-102 (tensors on `device`, scipy operators)."""
    with np.load(path, allow_pickle=True) as z:
        fr = {
            "V": torch.from_numpy(z["V"].astype("f")).to(device),
            "F": torch.from_numpy(z["F"].astype(np.int64)).to(device),
            "L": z["L"].item().astype("f").tocsr() if "L" in z else None,
            "Di": z["D"].item().astype("f").tocsr() if "D" in z else None,
            "DiA": z["DA"].item().astype("f").tocsr() if "DA" in z else None,
            "label": torch.from_numpy(z["label"]).to(device),
            "label_inv": torch.from_numpy(z["label_inv"]).to(device),
            "G": torch.from_numpy(z["dist_mat"].astype("f")).to(device),
        }
    return fr


def faust_frame_from_mesh(V, F, label=None, device="cuda", symmetric=True, geodesics="edges", laplacian="extrinsic",
                          component=None, repair=False) -> Dict:
    """The frame dict of load_faust_frame from a raw triangle mesh: V (nV, 3), F (nF, 3) (numpy or tensors), host scipy
    L / Di / DiA from mesh_ops.mesh_operators, and G — the `dist_mat` the reference's files bring along — computed on the device
    by operators.geodesic_matrix_from_mesh (geodesics="edges": edge-path distances, "triangles": paths that cross the faces;
    symmetric: min(D, D^T)).  label: the permutation of
    main.py:98-99 (vertex -> canonical id), None = identity.  A list of such frames is what FaustFrames takes.
    laplacian: "extrinsic" (default) keeps the host cotangent Laplacian; "intrinsic" takes L from the device builder on the
    intrinsic Delaunay triangulation (operators.laplacian_operator_from_mesh(intrinsic=True), fp32 scipy CSR) — the frame['L']
    the reference builds with mesh.intrinsic_laplacian (main.py:87), in this project's scaling, not the unpublished one.
    component: None (default) takes the mesh as it is; "largest" first runs operators.clean_mesh — the largest edge-connected
    component without bad faces and unused vertices, the reference's largest_component.py — builds the frame from the result
    and adds frame["vertex_map"] (new -> original vertex id).  label must then be None: a permutation of the original ids
    does not survive the removal, and the identity on the kept vertices is used.
    repair: True first runs operators.repair_mesh (duplicate vertices welded, duplicate faces dropped, every component wound
    consistently) — before component= and the builders — and adds frame["repair"], the RepairedMesh; frame["vertex_map"] then
    leads from the frame's vertices to the original ids through both steps.  label must be None here too."""
    from .operators import clean_mesh, geodesic_matrix_from_mesh, laplacian_operator_from_mesh, repair_mesh

    if geodesics not in ("edges", "triangles"):
        raise ValueError(f'faust_frame_from_mesh: geodesics must be "edges" or "triangles", got {geodesics!r}')
    if laplacian not in ("extrinsic", "intrinsic"):
        raise ValueError(f'faust_frame_from_mesh: laplacian must be "extrinsic" or "intrinsic", got {laplacian!r}')
    if component not in (None, "largest"):
        raise ValueError(f'faust_frame_from_mesh: component must be None or "largest", got {component!r}')
    vertex_map = repaired = None
    if repair:
        if label is not None:
            raise ValueError("faust_frame_from_mesh: repair=True renumbers the vertices; label must be None")
        Vt = V if torch.is_tensor(V) else torch.from_numpy(np.array(V, dtype=np.float32))
        Ft = F if torch.is_tensor(F) else torch.from_numpy(np.array(F))
        repaired = repair_mesh(Vt.to(device), Ft.to(device))
        V, F, vertex_map = repaired.V, repaired.F, repaired.vertex_map.to(torch.int64)
    if component == "largest":
        if label is not None:
            raise ValueError('faust_frame_from_mesh: component="largest" renumbers the vertices; label must be None')
        Vt = V if torch.is_tensor(V) else torch.from_numpy(np.array(V, dtype=np.float32))
        Ft = F if torch.is_tensor(F) else torch.from_numpy(np.array(F))
        cm = clean_mesh(Vt.to(device), Ft.to(device))
        kept = cm.vertex_map.to(torch.int64)
        V, F, vertex_map = cm.V, cm.F, kept if vertex_map is None else vertex_map[kept]
    Vn = np.asarray(V.detach().cpu() if torch.is_tensor(V) else V)
    Fn = np.asarray(F.detach().cpu() if torch.is_tensor(F) else F)
    nv = Vn.shape[0]
    label = np.arange(nv) if label is None else np.asarray(label.detach().cpu() if torch.is_tensor(label) else label)
    if label.shape != (nv,) or not np.array_equal(np.sort(label), np.arange(nv)):
        raise ValueError("faust_frame_from_mesh: label must be a permutation of the vertex ids")
    ops = mesh_ops.mesh_operators(Vn.astype(np.float32).astype(np.float64), Fn)
    Vd = torch.from_numpy(Vn.astype("f")).to(device)
    Fd = torch.from_numpy(Fn.astype(np.int64)).to(device)
    L = laplacian_operator_from_mesh(Vd, Fd, intrinsic=True).to_scipy() if laplacian == "intrinsic" else ops["L"]
    frame = {
        "V": Vd, "F": Fd, "L": L, "Di": ops["Di"], "DiA": ops["DiA"],
        "label": torch.from_numpy(label.astype(np.int64)).to(device),
        "label_inv": torch.from_numpy(np.argsort(label).astype(np.int64)).to(device),
        "G": geodesic_matrix_from_mesh(Vd, Fd, symmetric=symmetric, method=geodesics),
    }
    if vertex_map is not None:
        frame["vertex_map"] = vertex_map
    if repaired is not None:
        frame["repair"] = repaired
    return frame


def normal_frame_from_mesh(V, F, model="lap", uniform_mesh=True, hack=1, target="area", name=None, device="cuda", repair=False,
                           inputs=("V",), wks_k=300, curv_radius=5):
    """The frame dict of the reference's normal-prediction sampler (src/normal_predict/sampler.py:21-91, read_npz) from a raw
    triangle mesh, built on the device: {'V' (nV, 3) fp32, 'F' (nF, 3) int64, 'input' (= V), 'target_dist' (nV, 3), 'name'} and
    'L' (model="lap") or 'Di', 'DiA' (model="dir") as SparseOperators.
    uniform_mesh: V -= V.min(0); V /= V.max() (sampler.py:48-50) in float64, rounded to fp32.  target_dist: the unit vertex
    normals of the rescaled mesh, operators.vertex_normals(weighting=target) — the reference reads them from its OBJ files.
    L: the libigl-convention Laplacian M^-1 C with the barycentric mass and the clamp `hack`
    (operators.laplacian_operator_from_mesh(convention="libigl"); geom_utils.hacky_compute_laplacian).  Di / DiA: this project's
    operators.dirac_operators_from_mesh — the reference's igl.dirac_operator belongs to an unpublished fork and is not reproduced.
    Where read_npz gives up on a frame (non-finite target or operator values, sampler.py:31-33, 60-63, 75-77) this returns None
    after a warnings.warn naming the reason.
    repair: True first runs operators.repair_mesh on the mesh as given (welding, duplicate faces, one winding per component:
    what keeps the target normals from cancelling) and builds the frame from its result; the frame gains 'repair', the
    RepairedMesh with the maps back to the input.
    inputs: what 'input' holds, concatenated column-wise in the order given (train_4_normal.py:126's input table): "V" (3
    columns, the default: 'input' is then V itself) and "wks" (100 columns: operators.wave_kernel_signature of the rescaled
    mesh on the wks_k lowest eigenpairs, geom_utils.compute_wks; the reference uses 300).  With "wks" the frame gains
    'eigenpairs', the operators.Eigenpairs behind it.  "curv4" (4 columns: operators.curv4 of the rescaled mesh over
    curv_radius-ring patches, geom_utils.compute_curv4; the frame is None after its warning where curv4 is None, as read_npz
    gives up), "N" (3 columns: the area-weighted unit normals, compute_normals) and "G" (1 column: the raw angle defect,
    operators.gaussian_curvature(area_avg=False)).  Still missing of the reference's pipeline: the edge flips that
    fix_degenerate.py applies to zero-area faces (repair only counts those)."""
    import warnings

    from .operators import dirac_operators_from_mesh, laplacian_operator_from_mesh, repair_mesh, vertex_normals

    if model not in ("lap", "dir"):
        raise ValueError(f'normal_frame_from_mesh: model must be "lap" or "dir", got {model!r}')
    inputs = tuple(inputs)
    if not inputs or any(i not in ("V", "wks", "curv4", "N", "G") for i in inputs) or len(set(inputs)) != len(inputs):
        raise ValueError('normal_frame_from_mesh: inputs is a sequence of distinct names out of "V", "wks", "curv4", "N" and "G", '
                         f'got {inputs!r}')
    repaired = None
    if repair:
        Vt = V if torch.is_tensor(V) else torch.from_numpy(np.array(V, dtype=np.float32))
        Ft = F if torch.is_tensor(F) else torch.from_numpy(np.array(F))
        repaired = repair_mesh(Vt.to(device), Ft.to(device))
        V, F = repaired.V, repaired.F
    Vn = np.array(V.detach().cpu() if torch.is_tensor(V) else V, dtype=np.float32).astype(np.float64)
    Fn = np.asarray(F.detach().cpu() if torch.is_tensor(F) else F)
    if Vn.ndim != 2 or Vn.shape[1] != 3 or Fn.ndim != 2 or Fn.shape[1] != 3:
        raise ValueError(f"normal_frame_from_mesh wants V (nV, 3) and F (nF, 3), got {Vn.shape} and {Fn.shape}")
    if uniform_mesh and Vn.size:
        Vn = Vn - Vn.min(axis=0)
        Vn = Vn / Vn.max()
    Vd = torch.from_numpy(Vn.astype(np.float32)).to(device)
    Fd = torch.from_numpy(Fn.astype(np.int64)).to(device)

    def refuse(why):
        warnings.warn(f"normal_frame_from_mesh: {name if name is not None else 'mesh'}: {why}; no frame")
        return None

    target_dist = vertex_normals(Vd, Fd, weighting=target)
    if not bool(torch.isfinite(Vd).all()) or not bool(torch.isfinite(target_dist).all()):
        return refuse("non-finite coordinates or target normals")
    frame = {"V": Vd, "F": Fd, "input": Vd, "target_dist": target_dist, "name": name}
    if repaired is not None:
        frame["repair"] = repaired
    if model == "dir":
        if not mesh_ops.good_faces(Fn, Vn.shape[0]).all():      # the Dirac builder takes clean meshes only
            raise ValueError('normal_frame_from_mesh: model="dir" wants a mesh without bad faces (operators.clean_mesh makes one)')
        Di, DiA = dirac_operators_from_mesh(Vd, Fd)
        if not bool(torch.isfinite(Di._bsr4[2]).all()) or not bool(torch.isfinite(DiA._bsr4[2]).all()):
            return refuse("non-finite Dirac operator values")
        frame["Di"], frame["DiA"] = Di, DiA
    else:
        L = laplacian_operator_from_mesh(Vd, Fd, convention="libigl", mass="barycentric", hack=hack)
        if not bool(torch.isfinite(L.vals).all()):
            return refuse("non-finite Laplacian values")
        frame["L"] = L
    if inputs != ("V",):
        from .operators import laplacian_eigenpairs, wave_kernel_signature

        cols = {"V": Vd}
        if "wks" in inputs:
            frame["eigenpairs"] = laplacian_eigenpairs(Vd, Fd, k=wks_k)
            cols["wks"] = wave_kernel_signature(Vd, Fd, N=100, eigenpairs=frame["eigenpairs"])
        if "curv4" in inputs:
            from .operators import curv4

            cols["curv4"] = curv4(Vd, Fd.to(torch.int32), radius=curv_radius)
            if cols["curv4"] is None:
                return refuse("no principal curvatures")
        if "N" in inputs:
            cols["N"] = vertex_normals(Vd, Fd, weighting="area")
        if "G" in inputs:
            from .operators import gaussian_curvature

            cols["G"] = gaussian_curvature(Vd, Fd, area_avg=False).unsqueeze(1)
        frame["input"] = torch.cat([cols[i] for i in inputs], dim=1)
    return frame


def faust_from_files(paths: Sequence[str], device="cuda", model="lap", pad_to=None, reorder="auto", amplify="host"):
    """Resident FAUST dataset (dense_correspondence.FaustFrames) from reference .npz frames; `reorder` and `amplify` as
    FaustFrames."""
    from . import dense_correspondence as dc

    return dc.FaustFrames([load_faust_frame(p, device) for p in paths], model=model, pad_to=pad_to, device=device, reorder=reorder,
                          amplify=amplify)


def write_faust_frame(path: str, V: np.ndarray, F: np.ndarray, label: np.ndarray, dist_mat: np.ndarray) -> None:
    ops = mesh_ops.mesh_operators(V, F)
    wrap = lambda m: np.array(m, dtype=object)
    np.savez(path, V=V, F=F, L=wrap(ops["L"]), D=wrap(ops["Di"]), DA=wrap(ops["DiA"]), label=label,
             label_inv=np.argsort(label), dist_mat=dist_mat)
