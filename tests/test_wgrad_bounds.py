"""The side channel behind the two-piece fp16 weight gradient (sn_wgrad_*_bounded_f32), host side (no GPU):

* the table that carries a producer's maxima of |dy| between autograd nodes (kernels.note_absmax / take_absmax / clear_absmax):
  a bound is handed over once, only for exactly the memory it was noted for, and never after an in-place edit;
* the numpy model of the split (helpers.wgrad_split_model) and the premises of the probe operands that
  tests/test_wgrad_bounds_gpu.py feeds the kernel: where that file demands equality with float64, the model — h*h + h*l + l*h in
  fp32 — is itself exact, each of the three products is needed, and the dropped l*l is absent; where it demands the header's
  absolute error (include/sn_spmm.h, sn_wgrad_*_bounded_f32: 2^-39 of the bound), the model meets it.  Nothing here is fitted to
  a kernel's output."""
import gc
import weakref

import numpy as np
import pytest
import torch

from helpers import pow2_up_for, split_probe_operands, top_of_binade_operands, wgrad_split_model, wgrad_xbound
from surfacenetworks_amd import kernels


@pytest.fixture
def table():
    assert kernels._absmax_table == {}
    yield kernels._absmax_table
    kernels.clear_absmax()
    assert kernels._absmax_table == {}            # (tests/test_plans.py expects to find it empty)


def test_a_bound_is_taken_once(table):
    t, m = torch.randn(6, 4), torch.tensor([3.0, 1.0])
    kernels.note_absmax(t, m)
    assert kernels.take_absmax(t) is m
    assert kernels.take_absmax(t) is None and table == {}
    kernels.note_absmax(t, None)                  # a producer that left no maxima notes nothing
    assert table == {}


def test_an_in_place_edit_of_the_noted_tensor_drops_its_bound(table):
    t, m = torch.randn(6, 4), torch.tensor([3.0])
    kernels.note_absmax(t, m)
    t.mul_(2)
    assert kernels.take_absmax(t) is None and table == {}
    kernels.note_absmax(t, m)
    t.view(-1)[3:5].zero_()                       # through a view: the version counter is shared
    assert kernels.take_absmax(t) is None


def test_only_the_same_elements_get_the_bound(table):
    m = torch.tensor([3.0])
    t = torch.randn(4, 4)
    kernels.note_absmax(t, m)
    assert kernels.take_absmax(t[:3]) is None and table == {}       # same first element, fewer of them (the entry is spent)
    kernels.note_absmax(t, m)
    assert t.view(torch.int32).data_ptr() == t.data_ptr() and kernels.take_absmax(t.view(torch.int32)) is None
    kernels.note_absmax(t, m)
    tt = t.t()
    assert tt.data_ptr() == t.data_ptr() and tt.numel() == t.numel() and not tt.is_contiguous()
    assert kernels.take_absmax(tt) is None
    kernels.note_absmax(t, m)
    assert kernels.take_absmax(t[1:]) is None and len(table) == 1   # another first element: not even looked at
    assert kernels.take_absmax(t.reshape(2, 8)) is m                # a reshape of the same memory (autograd's view nodes) gets it
    kernels.note_absmax(t, m)
    assert kernels.take_absmax(t.detach().view(-1)) is m


def test_the_ninth_note_evicts_the_oldest_and_a_second_note_replaces_the_first(table):
    ts = [torch.randn(5) for _ in range(9)]
    ms = [torch.tensor([float(i)]) for i in range(9)]
    for t, m in zip(ts[:8], ms[:8]):
        kernels.note_absmax(t, m)
    assert len(table) == kernels._ABSMAX_KEEP == 8
    kernels.note_absmax(ts[8], ms[8])
    assert len(table) == 8
    assert kernels.take_absmax(ts[0]) is None                       # evicted
    for t, m in zip(ts[1:], ms[1:]):
        assert kernels.take_absmax(t) is m
    assert table == {}
    again = torch.tensor([7.0])
    kernels.note_absmax(ts[0], ms[0])
    kernels.note_absmax(ts[1], ms[1])
    kernels.note_absmax(ts[0], again)                               # same pointer: replaced, and now the youngest entry
    assert len(table) == 2 and list(table) == [ts[1].data_ptr(), ts[0].data_ptr()]
    assert kernels.take_absmax(ts[0]) is again


def test_clear_absmax_drops_the_references(table):
    t, m = torch.randn(6, 4), torch.tensor([3.0])
    rt, rm = weakref.ref(t), weakref.ref(m)
    kernels.note_absmax(t, m)
    del t, m
    gc.collect()
    assert rt() is not None and rm() is not None                    # the entry keeps the memory it describes alive
    kernels.clear_absmax()
    gc.collect()
    assert rt() is None and rm() is None and table == {}


# ---- the model of the split and the premises of the probe operands ----------------------------------------------------------
def test_scale_brings_every_bound_into_range():
    """pow2_up_for: a power of two that maps the bound into [2^14, 2^15) — below fp16's 65504 with a factor two to spare."""
    rng = np.random.default_rng(0)
    b = (rng.uniform(1.0, 2.0, 4000) * np.exp2(rng.integers(-60, 61, 4000))).astype(np.float32)
    b = np.concatenate([b, np.exp2(np.arange(-60, 61)).astype(np.float32), np.nextafter(np.exp2(np.arange(-60, 61)).astype(np.float32), np.float32(0))])
    s = pow2_up_for(b)
    assert (np.frexp(s)[0] == 0.5).all()
    scaled = b.astype(np.float64) * s
    assert (scaled >= 2.0 ** 14).all() and (scaled < 2.0 ** 15).all()
    assert np.isfinite(pow2_up_for(np.array([0.0, 1e-45, np.inf, np.nan], np.float32))).all()
    assert wgrad_xbound(np.array([0.5], np.float32), 1024)[0] == np.float32(32 * 1.0625 / 0.5)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [128, 256])
def test_probe_operands_meet_their_premises(C, seed):
    p = split_probe_operands(128, C, 70, 33, seed)
    got = wgrad_split_model(p["dy"], p["x"], p["center"], [p["bound"]], p["xinvstd"], p["stat_rows"]).astype(np.float64)
    ex = p["exact"]
    assert ex.sum() >= 18 * 18 and np.array_equal(got[ex], p["ref"][ex])             # three products in fp32: exact
    withll = wgrad_split_model(p["dy"], p["x"], p["center"], [p["bound"]], p["xinvstd"], p["stat_rows"], drop=("-ll",))
    assert np.array_equal(withll[ex].astype(np.float64), got[ex])                    # the dropped product is absent there
    err = np.abs(got - p["ref"])
    # (the unit the scale maps to 2^14 is <= the bound: |a - fp16 pieces| <= 2^-25 scaled = 2^-39 unit <= 2^-39 bound)
    assert p["loose_dy"].any() and (err <= 2.0 ** -39 * float(p["bound"]) * np.abs(p["x_row"])[None, :])[p["loose_dy"]].all()
    assert p["loose_x"].any() and (err <= 2.0 ** -39 * p["xbound"].astype(np.float64)[None, :] * np.abs(p["dy_row"])[:, None])[p["loose_x"]].all()


def test_every_retained_product_is_needed_by_some_exact_case():
    needed = {"hh": False, "hl": False, "lh": False}
    seen_k, seen_m = set(), set()
    for seed in range(4):
        p = split_probe_operands(128, 256, 40, 7, seed)
        ex = p["exact"]
        for name in needed:
            g = wgrad_split_model(p["dy"], p["x"], p["center"], [p["bound"]], p["xinvstd"], p["stat_rows"], drop=(name,))
            needed[name] |= bool((g.astype(np.float64)[ex] != p["ref"][ex]).any())
        # 22-bit elements all the way down to 2^-17 of the unit on either side
        seen_k |= set(p["k"][(p["kbits"] == 22) & ex.any(1)].tolist())
        seen_m |= set(p["m"][(p["mbits"] == 22) & ex.any(0)].tolist())
    assert all(needed.values()), needed
    assert set(range(1, 18)) <= seen_k and set(range(1, 18)) <= seen_m


def test_a_bound_that_is_too_small_or_too_large_shows_in_the_model():
    """What sections of the GPU file rely on: twenty binary orders of bound move the result in VALUE (too small: the scaled
    operand passes fp16's range; too large: the low bits fall off the denormal grid)."""
    p = split_probe_operands(128, 128, 40, 7, 0)
    ex = p["exact"]
    with np.errstate(over="ignore", invalid="ignore"):
        small = wgrad_split_model(p["dy"], p["x"], p["center"], [p["bound"] * np.float32(2.0 ** -20)], p["xinvstd"], p["stat_rows"])
    assert not np.isfinite(small).all()
    large = wgrad_split_model(p["dy"], p["x"], p["center"], [p["bound"] * np.float32(2.0 ** 20)], p["xinvstd"], p["stat_rows"])
    assert np.isfinite(large).all() and (large.astype(np.float64)[ex] != p["ref"][ex]).any()


@pytest.mark.parametrize("C", [128, 256])
def test_elements_at_a_bound_at_the_top_of_its_binade(C):
    """The premises of the device test of the same name: scaled, the bounds land within 2^-11 of 2^15 — finite in fp16, while one
    binary order more (a scale of 2^(16 - E)) would round them to infinity —, and the model keeps 22 significant bits of every
    element: 2^-22 of a product with a power of two, (3 + 2^-22) 2^-22 + 2 x 2^-24 (representation of both factors, the dropped
    l*l, two fp32 additions) of a product of two 24-bit factors."""
    p = top_of_binade_operands(128, C, 40, 7)
    sdy, sx = pow2_up_for(p["bound"]), pow2_up_for(p["xbound"])
    assert float(p["bound"]) * float(sdy.reshape(-1)[0]) < 2.0 ** 15 and (p["xbound"].astype(np.float64) * sx < 2.0 ** 15).all()
    with np.errstate(over="ignore"):
        assert np.isinf(np.float16(2 * float(p["bound"]) * float(sdy.reshape(-1)[0])))
        assert np.isinf((2 * p["xbound"] * sx).astype(np.float16)).all()
    G = wgrad_split_model(p["dy"], p["x"], p["center"], [p["bound"]], p["xinvstd"], p["stat_rows"]).astype(np.float64)
    err, ref = np.abs(G - p["ref"]), np.abs(p["ref"])
    assert np.isfinite(G).all()
    assert (err <= 2.0 ** -22 * ref)[:, p["pow2_x"]].all()
    assert (err <= ((3 + 2.0 ** -22) * 2.0 ** -22 + 2 * 2.0 ** -24) * ref).all()
