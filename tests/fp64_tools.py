"""The element-wise float64 criterion the kernel tests share (tests/test_head_kernels_gpu.py, tests/test_step_tail_gpu.py): the bound
of an fp32 reduction of K products, the NaN-sentinel and bit-pattern comparisons. Nothing here calls a project kernel."""
import torch

NAN = float("nan")
TINY = 1e-30


def tau(K):
    """Relative bound of an fp32 reduction over K products, in any order, with or without fma: 2 (K + 4) 2^-24, about twice
    gamma_K. K may be a tensor (a bound per row or per column)."""
    return 2.0 * (K + 4) * 2.0 ** -24


def within(got, ref, scale, K):
    """Element-wise |got - ref| <= tau(K) * scale + TINY in float64, scale = |A| @ |B| of the product (plus the magnitudes of
    whatever else the output adds up); a non-finite `got` fails."""
    got = got.detach().double().cpu()
    return torch.isfinite(got) & ((got - ref).abs() <= tau(K) * scale + TINY)


def assert_close(got, ref, scale, K, what):
    ok = within(got, ref, scale, K)
    if not bool(ok.all()):
        bad = (~ok).nonzero()[:4].tolist()
        g = got.detach().double().cpu()
        raise AssertionError("%s: %d of %d elements outside tau(K) |A||B|, first %s: got %s, want %s" % (
            what, int((~ok).sum()), ok.numel(), bad, [float(g[tuple(i)]) for i in bad], [float(ref[tuple(i)]) for i in bad]))


def all_nan(t):
    return bool(torch.isnan(t).all())


def same_bits(a, b):
    """Bit for bit (NaN sentinels included): floats compared as their int32 patterns."""
    if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)
