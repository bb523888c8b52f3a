"""``gf_subm_conv_apply_epilogue``'s refusals that come before any HIP call, on host buffers (no GPU): a half-present LayerNorm
pair, ``relu`` outside {0, 1}, a misaligned pointer, ``out`` overlapping an input, and what ``gf_subm_conv_apply_scratch`` refuses.
Each returns GF_EINVAL with the offending value named and leaves ``out`` untouched."""
import pytest
import torch

from gaussianformer_amd import _lib

GF_EINVAL = -1
N, B, SHAPE, K, CIN, COUT, PAIRS = 8, 1, (4, 4, 4), 3, 32, 32, 8
SENTINEL = 12345.0


class Host:
    """Host buffers of one call, every one its own 64-byte aligned allocation."""

    def __init__(self):
        lib = _lib.load()
        z = torch.zeros
        self.feat, self.weight = z(N, CIN), z(K ** 3, CIN, COUT)
        self.tables = z(int(lib.gf_subm_tables_bytes(N, B, *SHAPE, K)), dtype=torch.uint8)
        self.pair_in, self.partial = z(PAIRS, dtype=torch.int32), z(PAIRS, COUT)
        self.out = torch.full((N, COUT), SENTINEL)
        self.nscratch = int(lib.gf_subm_apply_scratch_bytes(N, CIN))
        self.scratch = z(self.nscratch, dtype=torch.uint8)
        self.bias, self.residual, self.ln_weight, self.ln_bias = z(COUT + 4), z(N, COUT), z(COUT), z(COUT)

    def call(self, relu=0, **over):
        """The entry point on the buffers' addresses; ``over``: an address (or ``None``) in place of a buffer's, or another size."""
        a = {k: getattr(self, k).data_ptr() for k in ("feat", "weight", "tables", "pair_in", "partial", "out", "scratch", "bias",
                                                      "residual", "ln_weight", "ln_bias")}
        a.update(N=N, Cin=CIN, Cout=COUT, K=K, nscratch=self.nscratch)
        a.update(over)
        lib = _lib.load()
        rc = lib.gf_subm_conv_apply_epilogue(a["N"], B, *SHAPE, a["K"], a["Cin"], a["Cout"], PAIRS, a["feat"], a["weight"], a["tables"],
                                             a["pair_in"], a["partial"], a["out"], a["scratch"], a["nscratch"], a["bias"],
                                             a["residual"], a["ln_weight"], a["ln_bias"], relu, None)
        return rc, lib.gf_last_error().decode()

    def untouched(self):
        return bool((self.out == SENTINEL).all())


def refused(h, needle, **kw):
    rc, msg = h.call(**kw)
    assert rc == GF_EINVAL, (rc, msg)
    assert "gf_subm_conv_apply_epilogue" in msg or "subm" in msg, msg
    assert needle in msg, msg
    assert h.untouched()


def test_half_present_norm_pair():
    h = Host()
    refused(h, "ln_bias", ln_bias=None)
    refused(h, "ln_weight", ln_weight=None)


def test_relu_outside_0_1():
    h = Host()
    refused(h, "relu = 2", relu=2)
    refused(h, "relu = -1", relu=-1)


@pytest.mark.parametrize("which", ["bias", "residual", "ln_weight", "ln_bias", "out"])
def test_misaligned_pointer(which):
    h = Host()
    refused(h, f"{which} = ", **{which: getattr(h, which).data_ptr() + 4})
    rc, msg = h.call(**{which: getattr(h, which).data_ptr() + 4})
    assert "16-byte aligned" in msg


@pytest.mark.parametrize("which", ["residual", "feat", "weight", "bias", "ln_weight", "ln_bias", "partial", "scratch"])
def test_out_aliasing_an_input(which):
    h = Host()
    name = "features" if which == "feat" else which
    refused(h, f"aliases {name}", out=getattr(h, which).data_ptr())


def test_out_overlapping_the_residuals_tail():
    h = Host()
    rows = torch.full((2 * N - 1, COUT), SENTINEL)      # out = rows[:N], residual = rows[N - 1:]: one row shared
    rc, msg = h.call(out=rows.data_ptr(), residual=rows[N - 1:].data_ptr())
    assert rc == GF_EINVAL and "aliases residual" in msg and bool((rows == SENTINEL).all())


def test_what_the_plain_entry_refuses():
    h = Host()
    refused(h, "scratch", scratch=None)
    refused(h, "scratch", nscratch=h.nscratch - 16)
    refused(h, "channels", Cout=48)
    refused(h, "kernel size", K=4)
    refused(h, "null pointer", feat=None)


def test_no_rows_is_ok_without_a_device():
    h = Host()
    rc, _ = h.call(N=0, relu=1)
    assert rc == 0 and h.untouched()
