"""The table that carries what finishes a raw face gradient from one Dirac block's backward to the previous one's
(kernels.note_tail / take_tail, beside the maxima table): host logic only, no GPU."""
import torch

from surfacenetworks_amd import kernels


def _tail(n):
    return tuple(torch.full((n,), float(k)) for k in range(3))


def test_a_tail_is_taken_only_for_the_same_memory_size_and_version():
    kernels.clear_absmax()
    base = torch.zeros(6, 4)
    tl = _tail(4)
    kernels.note_tail(base, tl)
    assert kernels.has_tail(base.view(2, 12)) and kernels.has_tail(base)            # (a view node of autograd: same memory)
    assert not kernels.has_tail(base[1:]) and kernels.take_tail(base[1:]) is None   # another first element
    assert kernels.take_tail(base.view(24)) is tl
    assert kernels.take_tail(base) is None                                         # taken once
    kernels.note_tail(base, tl)
    assert not kernels.has_tail(base[:3]) and kernels.take_tail(base[:3]) is None   # same first element, fewer elements
    assert kernels.take_tail(base) is None                                         # (and a failed take drops the entry)
    kernels.note_tail(base, tl)
    base.add_(1.0)                                                                 # an in-place edit: another version
    assert not kernels.has_tail(base) and kernels.take_tail(base) is None
    other = torch.zeros(6, 4)
    kernels.note_tail(base, tl)
    assert kernels.take_tail(other) is None and kernels.has_tail(base)
    kernels.clear_absmax()
    assert not kernels.has_tail(base) and kernels.take_tail(base) is None


def test_clear_absmax_empties_both_tables():
    t = torch.zeros(8)
    kernels.note_absmax(t, torch.ones(2))
    kernels.note_tail(t, _tail(8))
    assert kernels._absmax_table and kernels._tail_table
    kernels.clear_absmax()
    assert not kernels._absmax_table and not kernels._tail_table


def test_the_table_keeps_only_the_last_few_entries():
    kernels.clear_absmax()
    keep = [torch.zeros(4) for _ in range(kernels._ABSMAX_KEEP + 3)]
    for t in keep:
        kernels.note_tail(t, _tail(4))
    assert len(kernels._tail_table) == kernels._ABSMAX_KEEP
    assert not kernels.has_tail(keep[0]) and kernels.has_tail(keep[-1])
    kernels.clear_absmax()
