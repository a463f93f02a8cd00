"""TEST INFRASTRUCTURE: plain references for the transform tests (tests/test_gpu_transforms.py), written from the
definitions with numpy uint64 modular products and the oracle's NTT, plus the input generators and memory guards
the large-domain cases share.  The LDE reference takes any coset shift and log_blowup = 0, which orc.lde does not;
tests/test_transforms_reference.py pins it on orc.lde and on the sharded test double."""
import numpy as np

P = 3221225473


def mulmod(a, b):
    """Elementwise a * b mod P (canonical uint32 operands: the product fits 64 bits)."""
    return (np.asarray(a, dtype=np.uint64) * np.asarray(b, dtype=np.uint64) % P).astype(np.uint32)


def powers(x, count):
    """x^0 .. x^(count - 1) mod P as uint32, by doubling (log2(count) vector products)."""
    out = np.empty(count, dtype=np.uint64)
    out[0] = 1
    k = 1
    while k < count:
        m = min(k, count - k)
        out[k:k + m] = out[:m] * np.uint64(pow(int(x), k, P)) % P
        k += m
    return out.astype(np.uint32)


def rand_field(rng, n, chunk=1 << 24):
    """n uniform canonical residues, drawn directly as uint32 in chunks (no n-word uint64 temporary)."""
    out = np.empty(n, dtype=np.uint32)
    for i in range(0, n, chunk):
        out[i:i + chunk] = rng.integers(0, P, size=min(chunk, n - i), dtype=np.uint32)
    return out


def lde_ref(orc, trace, log_n, log_b, shift):
    """f(shift * h^i), i < 2^(log_n + log_b), of the interpolant of degree < n - 1 through the n - 1 trace values
    (the oracle's virtual point completes them): coefficients by orc.intt over g, coefficient k scaled by shift^k,
    zero-padded to N and transformed by orc.ntt over h.  What OracleBackend.lde computes, vectorised."""
    n, L = 1 << log_n, log_n + log_b
    t = np.ascontiguousarray(trace, dtype=np.uint32)
    assert len(t) == n - 1
    y = np.empty(n, dtype=np.uint32)
    y[:n - 1] = t
    y[n - 1] = orc.virtual_point(t, log_n)
    c = orc.intt(y, orc.gen_of_order_log(log_n))
    del y
    assert c[n - 1] == 0
    pad = np.zeros(1 << L, dtype=np.uint32)
    pad[:n] = mulmod(c, powers(shift, n))
    del c
    return orc.ntt(pad, orc.gen_of_order_log(L))


def linear_trace(log_n, c0, c1, chunk=1 << 24):
    """n words: t_i = q(g^i) = c0 + c1 g^i for i < n - 1 (g of order n), then a 0 (zk_dev_lde's trace layout).  The
    interpolant of degree < n - 1 through them is q itself, so its LDE is known without a transform."""
    n = 1 << log_n
    g = pow(5, (P - 1) >> log_n, P)
    gp = powers(g, min(chunk, n))
    t = np.empty(n, dtype=np.uint32)
    for i in range(0, n, len(gp)):
        t[i:i + len(gp)] = (mulmod(mulmod(gp, pow(g, i, P)), c1).astype(np.uint64) + c0) % P
    t[n - 1] = 0
    return t


def linear_lde_expected(t, log_n, c0, c1, shift, lo, hi):
    """f_i = q(shift g^i) for lo <= i < hi, log_blowup = 0, from the words of linear_trace:
    c0 + shift (t_i - c0), and f_{n-1} = c0 + shift c1 / g."""
    n = 1 << log_n
    f = ((t[lo:hi].astype(np.uint64) + (P - c0)) % P * shift % P + c0) % P
    if hi == n:
        f[-1] = (c0 + shift * c1 % P * pow(pow(5, (P - 1) >> log_n, P), P - 2, P)) % P
    return f.astype(np.uint32)


def mem_available():
    """Host MemAvailable in bytes (0 when /proc/meminfo cannot be read)."""
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) * 1024
    except OSError:
        pass
    return 0


def require_memory(device_bytes, host_bytes):
    """Skips the calling test, saying why, when the device or the host has less free memory than the case needs."""
    import pytest
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < device_bytes:
        pytest.skip(f"needs {device_bytes / 2**30:.0f} GiB of free device memory, {free / 2**30:.0f} GiB available")
    avail = mem_available()
    if avail < host_bytes:
        pytest.skip(f"needs {host_bytes / 2**30:.0f} GiB of available host memory, {avail / 2**30:.0f} GiB available")
