"""tests/memguard.py on CPU tensors: a write outside the slice, an element left unwritten, a wrong value and a modified input
are each reported; a correct slice write is not."""
import torch

import memguard as mg


def test_a_correct_write_passes_and_every_violation_is_reported():
    shape, idx = (2, 6, 3, 5), (slice(None), slice(2, 4))
    want = torch.randn(2, 2, 3, 5)
    g = mg.Guarded(shape, idx, "cpu")
    assert torch.isnan(g.view).all()
    g.view.copy_(want)
    assert g.problems(want, atol=0.0) == [] and g.problems(want, exact=True) == []
    assert g.bstride == 6 * 15

    g = mg.Guarded(shape, idx, "cpu")
    g.view.copy_(want)
    g.parent[1, 4, 0, 0] = 1.0                        # one channel past the slice, second image
    p = g.problems(want, atol=0.0)
    assert len(p) == 1 and "outside the slice" in p[0]

    g = mg.Guarded(shape, idx, "cpu")
    g.view.copy_(want)
    g.buf[-1] = 0.0                                    # the trailing guard band
    assert any("outside the slice" in s for s in g.problems(want, atol=0.0))

    g = mg.Guarded(shape, idx, "cpu")
    g.view.copy_(want)
    mg.poison_(g.view[0, 1, 2, 4:5])                   # one element never written
    p = g.problems()
    assert len(p) == 1 and "never written" in p[0] and "(0, 1, 2, 4)" in p[0]

    g = mg.Guarded(shape, idx, "cpu")
    g.view.copy_(want)
    g.view[1, 0, 1, 1] += 1e-3
    assert any("off the expected" in s for s in g.problems(want, atol=1e-4))
    assert g.problems(want, atol=2e-3) == []
    assert any("off the expected" in s for s in g.problems(want, exact=True))


def test_accumulate_mode_uint8_and_frozen_inputs():
    base = torch.randn(1, 3, 4, 4)
    g = mg.Guarded((1, 7, 4, 4), (slice(None), slice(4, 7)), "cpu", base=base)
    assert torch.equal(g.view, base)
    g.view.add_(1.0)
    assert g.problems(base + 1.0, atol=0.0) == []     # (no poison check in accumulate mode: the base is finite)

    u = mg.Guarded((2, 3, 2, 2), (slice(None), slice(0, 2)), "cpu", dtype=torch.uint8)
    u.view.fill_(4)
    assert u.problems(torch.full((2, 2, 2, 2), 4, dtype=torch.uint8), exact=True) == []
    u.parent[0, 2, 1, 1] = 4
    assert any("outside the slice" in s for s in u.problems())

    x = torch.randn(5)
    f = mg.Frozen(x)
    f.check()
    x[3] = -x[3]
    try:
        f.check("x")
    except AssertionError as e:
        assert "modified" in str(e)
    else:
        raise AssertionError("a modified input was not reported")
    ws = mg.poison_(torch.empty(64, dtype=torch.uint8))
    assert (ws == mg.POISON_U8).all()


def test_banded_allocation_reports_a_write_past_its_end():
    a = mg.Banded((3, 4), torch.float32, "cpu")
    assert a.t.shape == (3, 4) and torch.isnan(a.t).all() and a.intact()
    a.t.fill_(1.0)
    assert a.intact()
    a.buf[a.band + 12] = 0.0                           # one element past the payload
    assert not a.intact()
    u = mg.Banded((5,), torch.uint8, "cpu")
    assert (u.t == mg.POISON_U8).all() and u.intact()
    u.buf[u.band - 1] = 0
    assert not u.intact()


def test_reset_untouched_and_images_without_the_written_check():
    g = mg.Guarded((2, 3, 4), (slice(None), slice(1, 3)), "cpu")
    assert g.untouched()
    g.view.fill_(2.0)
    assert not g.untouched() and g.problems() == []
    g.reset()                                          # poison again: a second call starts from the same state
    assert g.untouched() and torch.isnan(g.view).all() and any("never written" in s for s in g.problems())
    g.parent[0, 0, 0] = 1.0                            # outside the slice: touched, and reset() restores the sentinel
    assert not g.untouched()
    g.reset()
    assert g.untouched() and g.problems(written=False) == []

    base = torch.randn(2, 2, 4)
    a = mg.Guarded((2, 3, 4), (slice(None), slice(1, 3)), "cpu", base=base)
    a.view.add_(1.0)
    a.reset()
    assert a.untouched() and torch.equal(a.view, base)

    u = mg.Guarded((16,), (Ellipsis,), "cpu", dtype=torch.uint8)     # a byte image: 0xFF is a value it may hold
    u.view[:8] = 3
    assert any("never written" in s for s in u.problems()) and u.problems(written=False) == []
    u.buf[0] = 0
    assert any("outside the slice" in s for s in u.problems(written=False))
    try:
        u.check(written=False, what="image")
    except AssertionError as e:
        assert "image" in str(e)
    else:
        raise AssertionError("a write into the band was not reported")
