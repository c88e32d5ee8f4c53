"""Host test of tests/scratch_guard.py: the detector detects, on the CPU, with three toy ops in plain torch that allocate
through a stand-in module patched exactly as the package's modules are (its `torch` global replaced by the proxy).

    a correct op                                  bitwise equal under all three patterns, guards intact
    an op that sums scratch whose tail it never wrote     its result differs between patterns
    an op that writes one element past its scratch        check() fails, with the site and the offset in the message"""
import re
import types

import pytest
import torch

import scratch_guard as sg

toy = types.ModuleType("toy_ops")            # the stand-in "package module": its ops reach torch through toy.torch alone
toy.torch = torch

N, PAD = 37, 64                              # 37 values in a scratch of 64: a ragged tile
POKE = torch.tensor([0x12345678], dtype=torch.int32).view(torch.float32)[0]       # no byte of it is a byte of a pattern


def op_correct(x):
    t = toy.torch
    scratch = t.empty(PAD, dtype=t.float32, device=x.device)
    scratch[:N] = x * 2.0
    scratch[N:] = 0.0                        # the producer writes its pad
    out = t.empty_like(x)
    out.copy_(scratch[:N] + scratch.sum())
    return out


def op_reads_unwritten_tail(x):
    t = toy.torch
    scratch = t.empty(PAD, dtype=t.float32, device=x.device)
    scratch[:N] = x * 2.0                    # ... and sums all 64: rows 37..63 are whatever the block held
    mask = t.zeros(PAD, device=x.device)
    mask[:N] = 1.0
    out = t.empty_like(x)
    out.copy_(scratch[:N] + (scratch * mask).sum())          # 0 * NaN is NaN; 0 * 3.39e38 is 0: a masked sum is no select
    return out


def op_writes_past_the_end(x):
    t = toy.torch
    scratch = t.empty(N, dtype=t.float32, device=x.device)   # <- the site the message must name
    wide = t.as_strided(scratch, (N + 1,), (1,))             # a "float4 tail store": one element too many
    wide[:N] = x
    wide[N] = POKE
    return scratch.clone()


def op_writes_in_front(x):
    t = toy.torch
    scratch = t.empty((N,), dtype=t.float32, device=x.device)
    whole = t.empty(0, dtype=t.float32).set_(scratch.untyped_storage(), scratch.storage_offset() - 2, (N + 2,), (1,))
    whole[0] = POKE
    whole[2:] = x
    return scratch.clone()


def _under(monkeypatch, op, x):
    outs = []
    for pat in sg.PATTERNS:
        with sg.guarded(toy, pat, monkeypatch, modules=[toy]) as g:
            outs.append(op(x).clone())
            assert g.check() >= 1
        assert toy.torch is torch                                # the proxy is gone with the block
    return outs


def _x():
    return torch.randn(N, generator=torch.Generator().manual_seed(5))


def test_correct_op_is_bitwise_equal_under_every_pattern_and_guards_hold(monkeypatch):
    x = _x()
    outs = _under(monkeypatch, op_correct, x)
    want = op_correct(x)                                         # unguarded
    assert all(torch.equal(o, want) for o in outs) and torch.isfinite(want).all()


def test_unwritten_tail_shows_as_a_difference_between_patterns(monkeypatch):
    x = _x()
    z, ff, big = _under(monkeypatch, op_reads_unwritten_tail, x)           # (guards intact: _under checked them)
    assert torch.isfinite(z).all() and torch.equal(z, x * 2.0 + (x * 2.0).sum())
    assert torch.isnan(ff).all()                                 # 0xFF..FF is a NaN: 0 * NaN
    assert not torch.equal(z, ff)
    # 0x7F7F7F7F = 3.39e38 is finite: a multiply by a zero mask hides it, as it hides zeros -- three patterns, not one
    assert torch.equal(z, big)


def test_write_past_the_end_trips_check_with_site_and_offset(monkeypatch):
    x = _x()
    line = op_writes_past_the_end.__code__.co_firstlineno + 2
    for pat in sg.PATTERNS:
        with pytest.raises(sg.GuardError) as e:
            with sg.guarded(toy, pat, monkeypatch, modules=[toy]):
                op_writes_past_the_end(x)
        msg = str(e.value)
        assert f"test_scratch_guard_host.py:{line}" in msg, msg
        assert re.search(rf"first changed byte at offset {4 * N} \(0 bytes past the end of a buffer of {4 * N} bytes", msg), msg
        assert toy.torch is torch                                # restored after a failure as well


def test_write_in_front_trips_check_with_a_negative_offset(monkeypatch):
    with pytest.raises(sg.GuardError, match=r"offset -8 \(8 bytes in front of a buffer of 148 bytes"):
        with sg.guarded(toy, 0x00, monkeypatch, modules=[toy]):
            op_writes_in_front(_x())


def test_explicit_check_inside_the_block(monkeypatch):
    with sg.guarded(toy, 0x7F, monkeypatch, modules=[toy]) as g:
        a = toy.torch.empty(3)
        assert g.check() == 1
        torch.as_strided(a, (4,), (1,))[3] = 0.0
        with pytest.raises(sg.GuardError):
            g.check()
        torch.as_strided(a, (4,), (1,))[3] = torch.tensor([0x7F7F7F7F], dtype=torch.int32).view(torch.float32)[0]


@pytest.mark.parametrize("pat", sg.PATTERNS)
def test_interior_is_aligned_filled_and_behaves_as_torch_empty(monkeypatch, pat):
    with sg.guarded(toy, pat, monkeypatch, modules=[toy]) as g:
        t = toy.torch
        assert t.float16 is torch.float16 and t.nn is torch.nn and t.zeros is torch.zeros          # forwarded
        cases = [t.empty(5), t.empty(3, 7), t.empty((3, 7)), t.empty([2, 3, 4], dtype=t.float16),
                 t.empty(torch.Size([4, 1])), t.empty((), dtype=t.float32), t.empty(0), t.empty(1001, dtype=t.uint8),
                 t.empty(2, 2, dtype=t.int64, device="cpu"), t.empty(6, dtype=t.bfloat16, device=torch.device("cpu")),
                 t.empty((2, 3, 4, 5), memory_format=t.channels_last), t.empty(3, requires_grad=True)]
        wants = [torch.empty(5), torch.empty(3, 7), torch.empty((3, 7)), torch.empty([2, 3, 4], dtype=torch.float16),
                 torch.empty(torch.Size([4, 1])), torch.empty((), dtype=torch.float32), torch.empty(0),
                 torch.empty(1001, dtype=torch.uint8), torch.empty(2, 2, dtype=torch.int64),
                 torch.empty(6, dtype=torch.bfloat16), torch.empty((2, 3, 4, 5), memory_format=torch.channels_last),
                 torch.empty(3, requires_grad=True)]
        src = [torch.zeros(4, 6), torch.zeros(4, 6, dtype=torch.float64).t(), torch.zeros(2, 3, 4, 5).permute(0, 2, 3, 1),
               torch.zeros(8, 8)[::2, ::2], torch.zeros(3, dtype=torch.int32)]
        for s in src:
            cases.append(t.empty_like(s))
            wants.append(torch.empty_like(s))
        cases += [t.empty_like(src[0], dtype=t.float16), t.empty_like(src[1], memory_format=t.contiguous_format),
                  t.empty_strided((3, 4), (1, 3), dtype=t.float64)]
        wants += [torch.empty_like(src[0], dtype=torch.float16),
                  torch.empty_like(src[1], memory_format=torch.contiguous_format),
                  torch.empty_strided((3, 4), (1, 3), dtype=torch.float64)]
        for got, want in zip(cases, wants):
            assert type(got) is torch.Tensor and got.shape == want.shape and got.dtype == want.dtype
            assert got.device == want.device and got.stride() == want.stride(), (got.shape, got.stride(), want.stride())
            assert got.requires_grad == want.requires_grad and got.is_leaf and not got._is_view()
            if got.numel():
                assert got.data_ptr() % sg.ALIGN == 0
                flat = torch.as_strided(got.detach(), (got.untyped_storage().nbytes() // got.element_size(),), (1,), 0)
                assert bool((flat.view(torch.uint8) == pat).all())           # interior and guards: all the pattern
            got.detach().zero_()                                              # the whole interior is writable ...
        assert g.check() == len(cases)                                        # ... without touching a guard
    assert len(g.buffers) == 0


def test_only_the_named_modules_see_the_proxy(monkeypatch):
    other = types.ModuleType("bystander")
    other.torch = torch
    with sg.guarded(toy, 0xFF, monkeypatch, modules=[toy]) as g:
        assert other.torch is torch and toy.torch is not torch
        a = torch.empty(4)                                                    # the test's own allocation: unguarded
        assert g.check() == 0 and a.untyped_storage().nbytes() == 16
    import sys
    assert sys.modules["torch"] is torch and torch.empty.__module__ is not None
