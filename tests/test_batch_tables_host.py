"""CPU tests of the helpers every GpuCodec method states its tensors with (vbz_compression_amd/batch.py: table, output, wrap_u32, ptr): a
table of the wrong dtype, a non-contiguous view, a tensor on another device and every wrong-shape rule raise AssertionError naming the table;
the exact case of each rule passes, more entries than n under the at-least rule included; an output is allocated as stated, a given one comes
back as the same object, and the three-state form does what its callers' docstrings say."""
import pytest
import torch

from vbz_compression_amd.batch import output, ptr, table, wrap_u32

CPU = torch.device("cpu")


def refused(name, *args, **kw):
    with pytest.raises(AssertionError) as e:
        table(name, *args, **kw)
    assert name in str(e.value), str(e.value)
    return str(e.value)


def test_dtype_contiguity_and_device():
    t = torch.zeros((4, 6), dtype=torch.int32)
    assert table("hits", t, torch.int32, CPU) is t and table("hits", t, torch.int32) is t
    msg = refused("hits", t, torch.float32, CPU)
    assert "torch.int32" in msg and "(4, 6)" in msg   # (the message carries the dtype and the shape)
    view = t[:, ::2]
    assert not view.is_contiguous()
    refused("hits", view, torch.int32, CPU)
    refused("hits", view, torch.int32)
    meta = torch.zeros((4, 6), dtype=torch.int32, device="meta")
    refused("hits", meta, torch.int32, CPU)
    assert table("hits", meta, torch.int32) is meta   # (no device stated: none checked)


def test_every_shape_rule():
    t = torch.zeros((3, 4), dtype=torch.int32)
    # the exact shape
    assert table("pairs", t, torch.int32, CPU, shape=(3, 4)) is t
    for shape in ((4, 3), (3, 5), (12,), (3, 4, 1)):
        refused("pairs", t, torch.int32, CPU, shape=shape)
    # free extents: dim() == 2 and shape[1] == 4; dim() == 2
    assert table("records", t, torch.int32, CPU, shape=(None, 4)) is t and table("ref", t, torch.int32, CPU, shape=(None, None)) is t
    refused("records", t, torch.int32, CPU, shape=(None, 3))
    refused("records", t.reshape(-1), torch.int32, CPU, shape=(None, 4))
    refused("ref", t.reshape(-1), torch.int32, CPU, shape=(None, None))
    # numel() == n, whatever the shape
    assert table("valid", t, torch.int32, CPU, numel=12) is t
    refused("valid", t, torch.int32, CPU, numel=11)
    refused("valid", t, torch.int32, CPU, numel=13)
    # numel() >= n
    assert table("scale", t, torch.int32, CPU, at_least=12) is t and table("scale", t, torch.int32, CPU, at_least=5) is t
    refused("scale", t, torch.int32, CPU, at_least=13)
    # an empty table
    e = torch.zeros((0, 4), dtype=torch.int32)
    assert table("records", e, torch.int32, CPU, shape=(None, 4)) is e and table("records", e, torch.int32, CPU, shape=(0, 4)) is e


def test_none():
    assert table("prior", None, torch.float32, CPU, shape=(2, 2), none=True) is None
    with pytest.raises(AssertionError) as e:
        table("valid", None, torch.int32, CPU, numel=2)
    assert "valid" in str(e.value)
    assert ptr(None) is None
    t = torch.zeros(3)
    assert ptr(t) == t.data_ptr()


def test_output_allocates_or_returns_the_callers():
    a = output("hit", None, torch.int32, CPU, (5, 4))
    assert a.dtype == torch.int32 and tuple(a.shape) == (5, 4) and a.device == CPU
    b = output("valid", None, torch.int64, CPU, 7)
    assert b.dtype == torch.int64 and tuple(b.shape) == (7,)
    assert output("hit", a, torch.int32, CPU, (5, 4)) is a
    assert output("valid", b, torch.int64, CPU, 7) is b
    two = torch.zeros((7, 1), dtype=torch.int64)
    assert output("valid", two, torch.int64, CPU, 7) is two   # (an entry count is a rule on numel(), not on the shape)
    for bad, dtype, shape in ((a, torch.int32, (4, 5)), (a.to(torch.float32), torch.int32, (5, 4)),
                              (torch.zeros((5, 8), dtype=torch.int32)[:, ::2], torch.int32, (5, 4)), (b, torch.int64, 6), (b, torch.int64, 8),
                              (torch.zeros((5, 4), dtype=torch.int32, device="meta"), torch.int32, (5, 4))):
        with pytest.raises(AssertionError) as e:
            output("hit", bad, dtype, CPU, shape)
        assert "hit" in str(e.value)
    # at least: a larger table passes, a smaller one does not
    assert output("start", b, torch.int64, CPU, 5, at_least=True) is b and output("start", b, torch.int64, CPU, 7, at_least=True) is b
    with pytest.raises(AssertionError):
        output("start", b, torch.int64, CPU, 8, at_least=True)
    assert tuple(output("start", None, torch.int64, CPU, 5, at_least=True).shape) == (5,)


def test_three_states():
    made = output("index", True, torch.int32, CPU, (2, 8), three_state=True)
    assert made.dtype == torch.int32 and tuple(made.shape) == (2, 8)
    assert output("index", False, torch.int32, CPU, (2, 8), three_state=True) is None
    assert output("index", None, torch.int32, CPU, (2, 8), three_state=True) is None   # (not wanted, as the callers' None always was)
    assert output("index", made, torch.int32, CPU, (2, 8), three_state=True) is made
    with pytest.raises(AssertionError) as e:
        output("index", made, torch.int32, CPU, (2, 9), three_state=True)
    assert "index" in str(e.value)


def test_the_uint32_wrap():
    got = wrap_u32([0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1])
    assert got.dtype == torch.int32 and got.tolist() == [0, 2147483647, -2147483648, -1]
    assert wrap_u32(torch.tensor([[2 ** 31, 5]], dtype=torch.int64)).tolist() == [-2147483648, 5]
    t = torch.tensor([3, -1], dtype=torch.int32)
    assert wrap_u32(t) is t
