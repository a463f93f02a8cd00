"""Host-side mirror of the reference interface, written over the C ABI (ctypes).

Names, argument meaning and error behaviour follow the reference so that tests
read like the reference's own (the reference panics; here a ZkError is raised).
"""
import ctypes as C
import struct

import numpy as np

from . import _lib
from ._lib import ZkError, check

P = 3221225473  # main.rs:13
# Merkle hash: the reference's SHA-256, the field-native one (configs[4]), or BLAKE2s-256 (RFC 7693; one compression per tree node).
# "blake2s" is taken by Context, Merkle, Proof.verify, compute_root_from_path, compute_root_from_coset and probe_hash_chain.
HASHES = {"sha256": 0, "field": 1, "blake2s": 2}


def _no_blake2s(who, hash):
    """BatchContext, Verifier and ShardContext have no BLAKE2s yet (their C setters refuse it too)."""
    if hash == "blake2s":
        raise ValueError(f"{who}: hash='blake2s' is not built for this class yet (Context, Merkle and Proof.verify take it)")


def _proof_data_len(o, log_batch=0, rows=False):
    """Bytes of a proof in the format of `o` (a Proof, Context, BatchContext or Verifier).  zk_proof_data_len_shared is the general
    entry point: log_batch 0 (one statement per proof), cap 0, stop 0 and one-value leaves are the older formats byte for byte.
    log_batch > 0: ONE shared proof of 2^log_batch statements (BatchContext.prove_shared); rows: with row leaves."""
    if getattr(o, "ext_log", 0):                    # challenges in E (Context(ext_log=1), Proof(ext_log=1)): one statement
        return _lib.load().zk_proof_data_len_ext(o.log_n, o.log_blowup, o.queries, o.grind_bits, o.fold_log, int(o.coset_leaves), o.stop_log, o.cap_log, o.ext_log)
    if rows:
        return _lib.load().zk_proof_data_len_shared_rows(o.log_n, o.log_blowup, o.queries, o.grind_bits, o.fold_log, int(o.coset_leaves), o.stop_log,
                                                         o.cap_log, log_batch, 1)
    return _lib.load().zk_proof_data_len_shared(o.log_n, o.log_blowup, o.queries, o.grind_bits, o.fold_log, int(o.coset_leaves), o.stop_log, o.cap_log,
                                                log_batch)


def _u32arr(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class field:
    """Scalar Gf<P> arithmetic (field.rs:8-211) on canonical residues."""
    P = P

    @staticmethod
    def add(a, b): return _lib.load().zk_field_add(a, b)
    @staticmethod
    def sub(a, b): return _lib.load().zk_field_sub(a, b)
    @staticmethod
    def mul(a, b): return _lib.load().zk_field_mul(a, b)
    @staticmethod
    def neg(a): return _lib.load().zk_field_neg(a)
    @staticmethod
    def inv(a): return _lib.load().zk_field_inv(a)
    @staticmethod
    def pow(a, e): return _lib.load().zk_field_pow(a, e)
    @staticmethod
    def from_u32(v): return _lib.load().zk_field_from_u32(v)
    @staticmethod
    def from_i32(v): return _lib.load().zk_field_from_i32(v)   # field.rs:10-18
    @staticmethod
    def div(a, b):                                             # field.rs:165-177; a zero divisor panics there
        if b % P == 0:
            raise ZeroDivisionError("Gf division by zero (field.rs:165-177)")
        return _lib.load().zk_field_div(a, b)
    @staticmethod
    def rem(a, rhs):                                           # field.rs:89-94
        if rhs == 0:
            raise ZeroDivisionError("Gf % 0 (field.rs:89-94)")
        return _lib.load().zk_field_rem(a, rhs)
    @staticmethod
    def generator(): return _lib.load().zk_field_generator()
    @staticmethod
    def root_of_unity(log_order): return _lib.load().zk_field_root_of_unity(log_order)
    @staticmethod
    def order(a): return _lib.load().zk_field_order(a)     # field.rs:45-49


def _ext_call(fn, *args):
    out = (C.c_uint32 * 2)()
    check(fn(*[(C.c_uint32 * 2)(a[0] & 0xFFFFFFFF, a[1] & 0xFFFFFFFF) if isinstance(a, (tuple, list)) else a for a in args], out))
    return (int(out[0]), int(out[1]))


def ext_mul(a, b):
    """Product in E = F_P[u] / (u^2 - 5) of the pairs (c0, c1) = c0 + c1 u (zk_ext_mul)."""
    return _ext_call(_lib.load().zk_ext_mul, tuple(a), tuple(b))


def ext_inv(a):
    """Inverse in E (zk_ext_inv); zero has none."""
    if a[0] % P == 0 and a[1] % P == 0:
        raise ZeroDivisionError("the inverse of zero in E")
    return _ext_call(_lib.load().zk_ext_inv, tuple(a))


def ext_pow(a, e):
    """a^e in E for an exponent 0 <= e < 2^64 (zk_ext_pow)."""
    return _ext_call(_lib.load().zk_ext_pow, tuple(a), C.c_uint64(e))


def host_hash_mode():
    """How the host thread hashes its share of the trees: 'portable' (then everything stays on the device),
    'sha-ni', or 'sha-ni + avx512 x16' (levels of >= 16 nodes sixteen at a time); zk_host_hash_mode."""
    return ("portable", "sha-ni", "sha-ni + avx512 x16")[_lib.load().zk_host_hash_mode()]


def probe_hash_chain(hash="sha256", waves_per_simd=4, hashes=16, launches=10, device=0):
    """Roofline probe (zk_probe_hash_chain): steady-state rate of the compiled inner hash in a dependent chain."""
    r = _lib.ChainProbe()
    check(_lib.load().zk_probe_hash_chain(device, HASHES[hash], waves_per_simd, hashes, launches, C.byref(r)))
    return {"ns_per_hash_per_simd": r.ns_per_hash_per_simd, "clock_ghz": r.clock_ghz, "ms": r.ms,
            "waves_per_simd": r.waves_per_simd, "launches": r.launches, "hashes": r.hashes, "cus": r.cus}


def trace_fibsq(count, a0=1, a1=3141592):
    """prover.rs:32-39."""
    out = np.zeros(count, dtype=np.uint32)
    check(_lib.load().zk_trace_fibsq(a0, a1, count, _ptr(out)))
    return out


def trace_fibsq_batch(a0s, a1s, count, device=0):
    """Many independent traces on the GPU, one lane each: returns [batch, count]."""
    a0s, a1s = _u32arr(a0s), _u32arr(a1s)
    out = np.zeros((len(a0s), count), dtype=np.uint32)
    check(_lib.load().zk_trace_fibsq_batch_host(device, _ptr(a0s), _ptr(a1s), len(a0s), count, _ptr(out)))
    return out


# ---- bincode 1.x default encoding of the types the prover commits ----
def encode(x):
    if isinstance(x, (bytes, bytearray)):          # Hash = [u8; 32]: raw
        return bytes(x)
    if isinstance(x, (int, np.integer)):           # u32
        return struct.pack("<I", int(x))
    if isinstance(x, list):                        # AuthPath = Box<[Hash]>
        return struct.pack("<Q", len(x)) + b"".join(bytes(h) for h in x)
    if isinstance(x, tuple):
        return b"".join(encode(e) for e in x)
    raise TypeError(f"cannot encode {type(x)}")


class Channel:
    """channel.rs:6-37."""

    def __init__(self):                              # channel.rs:12
        self._h = C.c_void_p()
        check(_lib.load().zk_channel_new(C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().zk_channel_free(self._h)
            self._h = None

    def commit(self, data):                          # channel.rs:19
        b = encode(data)
        check(_lib.load().zk_channel_commit(self._h, b, len(b)))

    def get_u32(self):                               # channel.rs:28
        v = C.c_uint32()
        check(_lib.load().zk_channel_get_u32(self._h, C.byref(v)))
        return v.value

    @property
    def state(self):
        out = C.create_string_buffer(32)
        check(_lib.load().zk_channel_state(self._h, out))
        return out.raw

    @property
    def data(self):
        n = _lib.load().zk_channel_data_len(self._h)
        out = C.create_string_buffer(max(n, 1))
        check(_lib.load().zk_channel_data(self._h, out, n))
        return out.raw[:n]

    def finalize(self, log_n=10, log_blowup=3, public_last=2338775057):   # channel.rs:34
        return Proof(self.state, self.data, log_n, log_blowup, public_last)


class Proof:
    """proof.rs:5-154.  verify() raises ZkError where the reference panics."""

    def __init__(self, state, data, log_n=10, log_blowup=3, public_last=2338775057, hash="sha256", queries=1, grind_bits=0,
                 fold_log=1, coset_leaves=False, stop_log=0, cap_log=0, ext_log=0):   # proof.rs:11
        self.state, self.data = bytes(state), bytes(data)
        self.ext_log = ext_log                       # challenges, cp and the FRI layers in E: zk_verify_ext, zk_proof_data_len_ext
        self.cap_log = cap_log                       # made with zk_ctx_set_merkle_cap: zk_verify_cap, zk_proof_data_len_cap
        self.stop_log = stop_log                     # made with zk_ctx_set_fri_stop: zk_verify_stop, zk_proof_data_len_stop
        self.log_n, self.log_blowup, self.public_last = log_n, log_blowup, public_last
        self.hash, self.queries, self.grind_bits, self.fold_log = hash, queries, grind_bits, fold_log
        self.coset_leaves = bool(coset_leaves)       # made with zk_ctx_set_coset_leaves: zk_verify_coset, zk_proof_data_len_coset

    def expected_len(self):
        """The length the format gives a proof of this shape."""
        return _proof_data_len(self)

    data_len = expected_len

    def _general(self):
        """Folded, coset-leaf, stopped and BLAKE2s proofs go through the general entry points (zk_verify_check and zk_verify_fold keep
        the two hashes they were defined with: a BLAKE2s proof of any setting is verified by zk_verify_stop)."""
        return self.fold_log != 1 or self.coset_leaves or self.stop_log or self.cap_log or self.hash == "blake2s" or self.ext_log

    def _verify_general(self, strict, out):
        if self.ext_log:                             # the one entry point that takes ext_log
            return _lib.load().zk_verify_ext(self.data, len(self.data), self.state if strict else None, self.log_n, self.log_blowup,
                                             self.public_last, HASHES[self.hash], self.queries, self.grind_bits, self.fold_log,
                                             int(self.coset_leaves), self.stop_log, self.cap_log, self.ext_log, C.byref(out))
        if self.cap_log:                             # Merkle caps: the one entry point that takes cap_log
            return _lib.load().zk_verify_cap(self.data, len(self.data), self.state if strict else None, self.log_n, self.log_blowup,
                                             self.public_last, HASHES[self.hash], self.queries, self.grind_bits, self.fold_log,
                                             int(self.coset_leaves), self.stop_log, self.cap_log, C.byref(out))
        if self.stop_log or self.hash == "blake2s":
            return _lib.load().zk_verify_stop(self.data, len(self.data), self.state if strict else None, self.log_n, self.log_blowup,
                                              self.public_last, HASHES[self.hash], self.queries, self.grind_bits, self.fold_log,
                                              int(self.coset_leaves), self.stop_log, C.byref(out))
        fn = _lib.load().zk_verify_coset if self.coset_leaves else _lib.load().zk_verify_fold
        return fn(self.data, len(self.data), self.state if strict else None, self.log_n, self.log_blowup,
                  self.public_last, HASHES[self.hash], self.queries, self.grind_bits, self.fold_log, C.byref(out))

    def verify(self, strict=False):                  # proof.rs:15
        """strict=True also replays the channel: challenges must come from the transcript and `state`
        must be its final state (the reference trusts the proof for both, proof.rs:22-37); with grind_bits > 0 it also
        checks the proof-of-work nonce."""
        if self._general():  # folded by 2^fold_log between commitments (zk_ctx_set_fold), coset leaves, early stop, BLAKE2s
            check(self._verify_general(strict, C.c_int32()))
            return
        if self.grind_bits:
            out = C.c_int32()
            check(_lib.load().zk_verify_grind(self.data, len(self.data), self.state if strict else None, self.log_n, self.log_blowup,
                                              self.public_last, HASHES[self.hash], self.queries, self.grind_bits, C.byref(out)))
            return
        check(_lib.load().zk_verify_queries(self.data, len(self.data), self.state if strict else None, self.log_n,
                                            self.log_blowup, self.public_last, HASHES[self.hash], self.queries))

    def check(self, strict=False):
        """The number of the check the CPU verifier stops at (zk_verify_grind): 0 = accepted; otherwise what verify()'s
        error names.  Never raises for a rejected proof."""
        out = C.c_int32()
        if self._general():
            rc = self._verify_general(strict, out)
        else:
            rc = _lib.load().zk_verify_grind(self.data, len(self.data), self.state if strict else None, self.log_n, self.log_blowup,
                                             self.public_last, HASHES[self.hash], self.queries, self.grind_bits, C.byref(out))
        if rc not in (_lib.ZK_OK, _ERR_VERIFY):
            check(rc)
        return out.value

    def size(self):                                  # proof.rs:151
        return _lib.load().zk_proof_size(len(self.data))


def compute_root_from_path(element, index, path, hash="sha256"):
    """merkle.rs:82-110."""
    flat = b"".join(bytes(h) for h in path)
    out = C.create_string_buffer(32)
    check(_lib.load().zk_compute_root_from_path_ex(element, index, flat, len(path), out, HASHES[hash]))
    return out.raw


def compute_root_from_coset(values, leaf, path, hash="sha256"):
    """zk_compute_root_from_coset: the root from the 1, 2, 4 or 8 slot values of coset leaf `leaf` and its path."""
    v = _u32arr(values)
    flat = b"".join(bytes(h) for h in path)
    out = C.create_string_buffer(32)
    check(_lib.load().zk_compute_root_from_coset(_ptr(v), len(v), leaf, flat, len(path), out, HASHES[hash]))
    return out.raw


class Merkle:
    """merkle.rs:6-79: SHA-256 heap built on the GPU; merkle[i], merkle.trace(i)."""

    def __init__(self, size, data, device=0, hash="sha256"):        # Merkle::new, merkle.rs:14
        vals = _u32arr(list(data) if not isinstance(data, np.ndarray) else data)
        if len(vals) != size:
            raise ZkError(-1, f"Merkle.new: size {size} != len(data) {len(vals)}")
        self.size = size
        self.nodes = np.zeros((max(2 * size - 1, 1), 32), dtype=np.uint8)
        check(_lib.load().zk_merkle_build_host_ex(device, _ptr(vals), size, _ptr(self.nodes), HASHES[hash]))

    new = classmethod(lambda cls, size, data, device=0, hash="sha256": cls(size, data, device, hash))

    def __getitem__(self, i):                        # merkle.rs:74-79
        return bytes(self.nodes[i])

    def __len__(self):
        return len(self.nodes)

    def trace(self, i):                              # merkle.rs:54-71
        i += len(self.nodes) // 2
        v = []
        while i != 0:
            if i % 2 == 0:
                v.append(self[i - 1]); i -= 2
            else:
                v.append(self[i + 1]); i -= 1
            i >>= 1
        return v


def ntt(data, inverse=False, device=0):
    """Natural-order NTT of size 2^k with root field.root_of_unity(k)."""
    a = _u32arr(data).copy()
    k = int(len(a)).bit_length() - 1
    if len(a) != 1 << k:
        raise ZkError(-1, "ntt: length must be a power of two")
    check(_lib.load().zk_ntt_host(device, _ptr(a), k, 1 if inverse else 0))
    return a


def lde(trace, log_n, log_blowup, device=0):
    """lagrange + solve over the coset (prover.rs:60-70) as one call."""
    t = _u32arr(trace)
    out = np.zeros(1 << (log_n + log_blowup), dtype=np.uint32)
    check(_lib.load().zk_lde_host(device, _ptr(t), log_n, log_blowup, _ptr(out)))
    return out


def _read_nodes(fn, handle, tree, heap, first, count):
    if count is None:
        count = max(heap - first, 0)
    out = np.zeros((count, 32), dtype=np.uint8)
    check(fn(handle, tree, first, count, out.ctypes.data_as(C.c_void_p)))
    return out


class Context:
    """Device-resident prover state for one (log_n, log_blowup): zk_ctx."""

    def __init__(self, log_n=10, log_blowup=3, device=0, hash="sha256", queries=1, host_levels=None, grind_bits=0, fold_log=1,
                 coset_leaves=False, stop_log=0, cap_log=0, ext_log=0):
        """ext_log: 1 draws the challenges, and holds cp and the FRI layers, in the quadratic extension E (zk_ctx_set_ext; 0 = the base field).
        cap_log: commit every tree by its 2^cap_log digests of depth cap_log and open paths that much shorter (zk_ctx_set_merkle_cap;
        0 = roots).  host_levels: (top_log, tail_log) of zk_ctx_set_host_levels; None = the library default.  grind_bits: proof-of-work
        bits before the query draw (zk_ctx_set_grinding; 0 = none).  fold_log: FRI folding factor 2^fold_log between commitments
        (zk_ctx_set_fold; 1 = the reference).  coset_leaves: one coset per Merkle leaf of the FRI trees (zk_ctx_set_coset_leaves).
        stop_log: stop FRI at a polynomial of degree < 2^stop_log and send its coefficients (zk_ctx_set_fri_stop; 0 = fold to a constant)."""
        self.fold_log = fold_log
        self.coset_leaves = False
        self.stop_log = 0
        self.cap_log = 0
        self.ext_log = 0
        self.log_n, self.log_blowup, self.device, self.hash, self.queries = log_n, log_blowup, device, hash, queries
        self.grind_bits = grind_bits
        self.n, self.B = 1 << log_n, 1 << log_blowup
        self.N, self.rounds = self.n * self.B, log_n
        self._h = C.c_void_p()
        check(_lib.load().zk_ctx_create(device, log_n, log_blowup, C.byref(self._h)))
        if hash != "sha256":
            check(_lib.load().zk_ctx_set_hash(self._h, HASHES[hash]))
        if queries != 1:
            check(_lib.load().zk_ctx_set_queries(self._h, queries))
        if host_levels is not None:
            check(_lib.load().zk_ctx_set_host_levels(self._h, host_levels[0], host_levels[1]))
        if grind_bits:
            check(_lib.load().zk_ctx_set_grinding(self._h, grind_bits))
        if fold_log != 1:
            check(_lib.load().zk_ctx_set_fold(self._h, fold_log))
        if coset_leaves:
            self.set_coset_leaves(True)
        if stop_log:
            self.set_fri_stop(stop_log)
        if cap_log:
            self.set_merkle_cap(cap_log)
        if ext_log:
            self.set_ext(ext_log)

    def set_ext(self, ext_log):
        """zk_ctx_set_ext: from the next proof on, challenges in E = F_P[u] / (u^2 - 5) (1) or in the base field (0).  Sizes the second planes of
        the layers and the decommitment buffers when called; refused (ZK_ERR_STATE) while a proof runs on the context."""
        check(_lib.load().zk_ctx_set_ext(self._h, ext_log))
        self.ext_log = ext_log

    def ext_challenges(self):
        """The component-1 raws of the last proof's challenges: three alphas, then one per group (zk_ctx_ext_challenges)."""
        out, n = (C.c_uint32 * 64)(), C.c_size_t()
        check(_lib.load().zk_ctx_ext_challenges(self._h, out, 64, C.byref(n)))
        return [int(out[i]) for i in range(n.value)]

    def set_merkle_cap(self, cap_log):
        """zk_ctx_set_merkle_cap: from the next one-call proof on, a tree of 2^lg leaves is committed by the 2^ce digests of depth
        ce = min(cap_log, lg - 1) and its paths carry lg - ce digests (0: roots, the reference)."""
        check(_lib.load().zk_ctx_set_merkle_cap(self._h, cap_log))
        self.cap_log = cap_log

    def merkle_cap(self, tree):
        """zk_ctx_merkle_cap: the digests the last one-call proof committed for `tree`, a [2^ce, 32] uint8 array (ce = 0: the root)."""
        out = np.zeros((1 << _lib.load().zk_ctx_merkle_cap_log(self._h, tree), 32), dtype=np.uint8)
        check(_lib.load().zk_ctx_merkle_cap(self._h, tree, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def set_coset_leaves(self, on=True):
        """zk_ctx_set_coset_leaves: from the next proof on, a group opens one leaf of 2^steps values and one path."""
        check(_lib.load().zk_ctx_set_coset_leaves(self._h, int(bool(on))))
        self.coset_leaves = bool(on)

    def set_fri_stop(self, stop_log):
        """zk_ctx_set_fri_stop: from the next proof on, fold only log_n - stop_log rounds and commit the 2^stop_log coefficients of the
        polynomial left (0: fold down to a constant, the reference)."""
        check(_lib.load().zk_ctx_set_fri_stop(self._h, stop_log))
        self.stop_log = stop_log

    def final_poly(self):
        """zk_ctx_final_poly: the coefficients the last proof ended with (stop_log 0: one value, the free term); with ext_log = 1 the words
        of both planes in wire order, 2 * 2^stop_log of them."""
        out, n = np.zeros(2 << 8, dtype=np.uint32), C.c_size_t()
        check(_lib.load().zk_ctx_final_poly(self._h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def fri_final_poly(self, layer, bound):
        """zk_fri_final_poly: (coefficients of the interpolant of FRI layer `layer`, number of non-zero ones of degree >= bound)."""
        out, high = np.zeros(self.layer_size(layer), dtype=np.uint32), C.c_uint32()
        check(_lib.load().zk_fri_final_poly(self._h, layer, bound, _ptr(out), C.byref(high)))
        return out, high.value

    def _proof_cap(self):
        return _proof_data_len(self)

    def set_fold(self, fold_log):
        """zk_ctx_set_fold: fold by 2^fold_log (1..3) between commitments from the next proof on."""
        check(_lib.load().zk_ctx_set_fold(self._h, fold_log))
        self.fold_log = fold_log

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().zk_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    @property
    def setup_ms(self): return _lib.load().zk_ctx_setup_ms(self._h)
    @property
    def device_bytes(self): return _lib.load().zk_ctx_device_bytes(self._h)
    @property
    def stream(self): return _lib.load().zk_ctx_stream(self._h)

    @property
    def host_levels(self):
        a, b = C.c_uint32(), C.c_uint32()
        check(_lib.load().zk_ctx_get_host_levels(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def sync(self): check(_lib.load().zk_ctx_sync(self._h))
    def set_profiling(self, classes=()):
        """Time the named kernel classes (_lib.KERNEL_CLASSES) with HIP events; () = off, "all" = every class."""
        if classes == "all":
            classes = _lib.KERNEL_CLASSES
        mask = 0
        for c in classes:
            mask |= 1 << _lib.KERNEL_CLASSES.index(c)
        check(_lib.load().zk_ctx_set_profiling(self._h, mask))

    def kernel_stats(self, reset=True):
        arr = _lib.kernel_stat_array()
        check(_lib.load().zk_kernel_stats(self._h, arr, len(arr), int(reset)))
        return {name: {"launches": int(a.launches), "ms": a.ms, "bytes": a.bytes, "ops": a.ops}
                for name, a in zip(_lib.KERNEL_CLASSES, arr)}

    def layer_size(self, layer): return self.N if layer == 0 else self.N >> (layer - 1)

    def trace_upload(self, trace):
        t = _u32arr(trace)
        check(_lib.load().zk_trace_upload(self._h, _ptr(t), len(t)))

    def lde(self): check(_lib.load().zk_lde(self._h))

    def merkle_commit(self, layer, coset_steps=0):
        """coset_steps > 0: leaves of 2^coset_steps values (zk_merkle_commit_coset); the tree then has layer_size >> coset_steps leaves."""
        out = C.create_string_buffer(32)
        if coset_steps:
            check(_lib.load().zk_merkle_commit_coset(self._h, layer, coset_steps, out))
            return out.raw
        check(_lib.load().zk_merkle_commit(self._h, layer, out))
        return out.raw

    def compose(self, alpha_raw):
        a = _u32arr(alpha_raw)
        check(_lib.load().zk_compose(self._h, _ptr(a)))

    def fri_fold(self, rnd, beta_raw): check(_lib.load().zk_fri_fold(self._h, rnd, beta_raw))

    def fri_fold_multi(self, rnd, steps, beta_raw):
        """zk_fri_fold_multi: layer 1 + rnd -> layer 1 + rnd + steps in one pass (challenges beta, beta^2, beta^4)."""
        check(_lib.load().zk_fri_fold_multi(self._h, rnd, steps, beta_raw))

    def layer_read(self, layer, offset=0, count=None):
        if count is None:
            count = self.layer_size(layer) - offset
        out = np.zeros(count, dtype=np.uint32)
        check(_lib.load().zk_layer_read(self._h, layer, offset, count, _ptr(out)))
        return out

    def layer_write(self, layer, values, offset=0):
        v = _u32arr(values)
        check(_lib.load().zk_layer_write(self._h, layer, offset, len(v), _ptr(v)))

    def merkle_node(self, tree, index):
        out = C.create_string_buffer(32)
        check(_lib.load().zk_merkle_node(self._h, tree, index, out))
        return out.raw

    def merkle_nodes(self, tree, first=0, count=None, coset_steps=0):
        """Nodes [first, first + count) of tree `tree` (default: the whole heap) as a [count, 32] uint8 array, in one copy.
        coset_steps: what the tree was built with (its heap has 2 (layer_size >> coset_steps) - 1 nodes)."""
        return _read_nodes(_lib.load().zk_merkle_nodes, self._h, tree, 2 * (self.layer_size(tree) >> coset_steps) - 1, first, count)

    def merkle_path(self, tree, leaf):
        buf = C.create_string_buffer(32 * 64)
        n = C.c_size_t()
        check(_lib.load().zk_merkle_path(self._h, tree, leaf, buf, C.byref(n)))
        return [buf.raw[32 * i:32 * i + 32] for i in range(n.value)]

    def prove(self, trace=None):
        """generate_proof as one C call (C++ host prover). trace=None: already uploaded."""
        cap = self._proof_cap()
        buf = C.create_string_buffer(cap)
        st = C.create_string_buffer(32)
        n = C.c_size_t()
        if trace is None:
            check(_lib.load().zk_prove_resident(self._h, buf, cap, C.byref(n), st))
        else:
            t = _u32arr(trace)
            check(_lib.load().zk_prove(self._h, _ptr(t), len(t), buf, cap, C.byref(n), st))
        info = self.last_transcript()
        return Proof(st.raw, buf.raw[:n.value], self.log_n, self.log_blowup, info.public_last, self.hash, self.queries, self.grind_bits,
                     self.fold_log, self.coset_leaves, self.stop_log, self.cap_log, self.ext_log)

    def prove_channel(self, channel):
        """generate_proof(channel) (prover.rs:9) in one C call on the caller's Channel (zk_prove_channel): the
        resident trace is proved on top of whatever the channel already holds; returns channel.finalize(...)."""
        check(_lib.load().zk_prove_channel(self._h, channel._h))
        proof = channel.finalize(self.log_n, self.log_blowup, self.last_transcript().public_last)
        proof.grind_bits, proof.fold_log, proof.coset_leaves = self.grind_bits, self.fold_log, self.coset_leaves
        proof.stop_log, proof.cap_log, proof.ext_log = self.stop_log, self.cap_log, self.ext_log
        return proof

    def set_host_levels(self, top_log, tail_log):
        check(_lib.load().zk_ctx_set_host_levels(self._h, top_log, tail_log))

    def set_early_launch(self, on=True):
        """zk_ctx_set_early_launch: the next FRI round's launches are enqueued before the current commitment is waited for."""
        check(_lib.load().zk_ctx_set_early_launch(self._h, int(on)))
        return bool(_lib.load().zk_ctx_get_early_launch(self._h))

    def set_checks(self, on=True):
        """The reference's in-prover assertions (prover.rs:64-66, :148-159/:169, :228-251) inside prove()."""
        check(_lib.load().zk_ctx_set_checks(self._h, int(on)))

    def last_transcript(self):
        """zk_transcript_info of the last proof: challenges, roots, and with grinding grind_bits and grind_nonce."""
        info = _lib.TranscriptInfo()
        check(_lib.load().zk_last_transcript(self._h, C.byref(info)))
        return info


def grind(state, bits, start=0, device=0):
    """zk_grind: the smallest nonce >= start whose SHA-256(state || le64(nonce)) begins with `bits` zero bits, searched on the GPU."""
    out = C.c_uint64()
    check(_lib.load().zk_grind(device, bytes(state), bits, start, C.byref(out)))
    return out.value


def grind_host(state, bits, start=0, threads=16):
    """zk_grind_host: the same search on <= 16 host threads (the same nonce)."""
    out = C.c_uint64()
    check(_lib.load().zk_grind_host(bytes(state), bits, start, threads, C.byref(out)))
    return out.value


def prove_many(ctxs):
    """Context.prove() (resident traces) on several contexts at once, one host thread each inside the
    library (zk_prove_many): returns the proofs in order."""
    ctxs = list(ctxs)
    c0 = ctxs[0]
    stride = max(c._proof_cap() for c in ctxs)
    handles = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    data = np.zeros((len(ctxs), stride), dtype=np.uint8)
    lens = (C.c_size_t * len(ctxs))()
    states = np.zeros((len(ctxs), 32), dtype=np.uint8)
    check(_lib.load().zk_prove_many(handles, len(ctxs), data.ctypes.data_as(C.c_void_p), stride, lens, states.ctypes.data_as(C.c_void_p)))
    out = []
    for i, c in enumerate(ctxs):
        out.append(Proof(states[i].tobytes(), data[i, :lens[i]].tobytes(), c.log_n, c.log_blowup, c.last_transcript().public_last,
                         c.hash, c.queries, c.grind_bits, c.fold_log, c.coset_leaves, c.stop_log, c.cap_log, c.ext_log))
    return out


class BatchContext:
    """2^log_batch proofs of one size in lockstep (zk_batch_*): every stage is one
    launch over the whole batch; each proof has its own channel and is byte-identical to Context.prove()."""

    def __init__(self, log_n=10, log_blowup=3, log_batch=4, device=0, hash="sha256", queries=1, grind_bits=0, fold_log=1, coset_leaves=False,
                 stop_log=0, cap_log=0, shared_rows=False, ext_log=0):
        """ext_log: 1 draws every proof's challenges, and holds cp and the FRI layers, in the quadratic extension E (zk_batch_set_ext;
        0 = the base field); prove() then returns Proofs with ext_log = 1, prove_shared() is refused.
        shared_rows: prove_shared() commits the traces as row leaves, one f tree and three f paths per query (zk_batch_set_shared_rows).
        fold_log: FRI folding factor 2^fold_log between commitments for every proof of the batch (zk_batch_set_fold; 1 = the
        reference).  coset_leaves: one coset per Merkle leaf of the FRI trees (zk_batch_set_coset_leaves).  stop_log: every proof stops
        FRI at a polynomial of degree < 2^stop_log and sends its coefficients (zk_batch_set_fri_stop; 0 = fold to a constant).
        cap_log: every proof commits each tree by its 2^cap_log digests of depth cap_log and opens paths that much shorter
        (zk_batch_set_merkle_cap; 0 = roots)."""
        _no_blake2s("BatchContext", hash)
        self.log_n, self.log_blowup, self.log_batch, self.hash, self.queries = log_n, log_blowup, log_batch, hash, queries
        self.grind_bits, self.fold_log = grind_bits, 1
        self.coset_leaves = False
        self.stop_log = 0
        self.cap_log = 0
        self.ext_log = 0
        self.shared_rows = False
        self.n, self.batch = 1 << log_n, 1 << log_batch
        self._h = C.c_void_p()
        check(_lib.load().zk_batch_create(device, log_n, log_blowup, log_batch, C.byref(self._h)))
        if hash != "sha256":
            check(_lib.load().zk_batch_set_hash(self._h, HASHES[hash]))
        if queries != 1:
            check(_lib.load().zk_batch_set_queries(self._h, queries))
        if grind_bits:
            check(_lib.load().zk_batch_set_grinding(self._h, grind_bits))
        if fold_log != 1:
            self.set_fold(fold_log)
        if coset_leaves:
            self.set_coset_leaves(True)
        if stop_log:
            self.set_fri_stop(stop_log)
        if cap_log:
            self.set_merkle_cap(cap_log)
        if shared_rows:
            self.set_shared_rows(True)
        if ext_log:
            self.set_ext(ext_log)

    def set_ext(self, ext_log):
        """zk_batch_set_ext: from the next zk_batch_prove on, challenges in E = F_P[u] / (u^2 - 5) (1) or in the base field (0).  Sizes the
        planes of the layers, the gather buffers and the tables of E when called, both ways; ZkError for ext_log > 1 or while a prove runs."""
        check(_lib.load().zk_batch_set_ext(self._h, ext_log))
        self.ext_log = ext_log

    def set_shared_rows(self, on=True):
        """zk_batch_set_shared_rows: from the next prove_shared() on, the 2^log_batch trace polynomials are committed as ONE tree whose leaf i
        holds the row (f_0[i], .., f_{M-1}[i]); a query opens three rows and three paths whatever the batch.  prove() does not look at it."""
        check(_lib.load().zk_batch_set_shared_rows(self._h, int(bool(on))))
        self.shared_rows = bool(_lib.load().zk_batch_get_shared_rows(self._h))

    def set_merkle_cap(self, cap_log):
        """zk_batch_set_merkle_cap: from the next zk_batch_prove on, every proof commits a tree of 2^lg leaves by the 2^ce digests of
        depth ce = min(cap_log, lg - 1) and its paths carry lg - ce digests (0: roots, the reference)."""
        check(_lib.load().zk_batch_set_merkle_cap(self._h, cap_log))
        self.cap_log = cap_log

    def merkle_cap(self, tree, proof):
        """zk_batch_merkle_cap: the digests proof `proof` of the last prove committed for `tree`, a [2^ce, 32] uint8 array (ce = 0: its root)."""
        out = np.zeros((1 << _lib.load().zk_batch_merkle_cap_log(self._h, tree), 32), dtype=np.uint8)
        check(_lib.load().zk_batch_merkle_cap(self._h, tree, proof, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def set_fri_stop(self, stop_log):
        """zk_batch_set_fri_stop: from the next zk_batch_prove on, every proof folds only log_n - stop_log rounds and commits the
        2^stop_log coefficients of its final polynomial (0 = fold down to a constant)."""
        check(_lib.load().zk_batch_set_fri_stop(self._h, stop_log))
        self.stop_log = stop_log

    def set_fold(self, fold_log):
        """zk_batch_set_fold: fold by 2^fold_log (1..3) between commitments from the next zk_batch_prove on."""
        check(_lib.load().zk_batch_set_fold(self._h, fold_log))
        self.fold_log = fold_log

    def set_coset_leaves(self, on=True):
        """zk_batch_set_coset_leaves: from the next zk_batch_prove on, a group opens one leaf of 2^steps values and one path."""
        check(_lib.load().zk_batch_set_coset_leaves(self._h, int(bool(on))))
        self.coset_leaves = bool(on)

    @property
    def proof_len(self):
        return _proof_data_len(self)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().zk_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    @property
    def device_bytes(self): return _lib.load().zk_batch_device_bytes(self._h)

    def set_traces(self, traces):
        """traces: [batch][n-1] canonical residues."""
        t = np.ascontiguousarray(traces, dtype=np.uint32)
        if t.shape != (self.batch, self.n - 1):
            raise ZkError(-1, f"expected traces of shape ({self.batch}, {self.n - 1})")
        check(_lib.load().zk_batch_set_traces(self._h, _ptr(t)))

    def gen_fibsq(self, a0s, a1s):
        """prover.rs:32-39 for every proof, on the device, from the seeds a0s[p], a1s[p]."""
        a0, a1 = _u32arr(a0s), _u32arr(a1s)
        if len(a0) != self.batch or len(a1) != self.batch:
            raise ZkError(-1, f"expected {self.batch} seeds")
        check(_lib.load().zk_batch_gen_fibsq(self._h, _ptr(a0), _ptr(a1)))

    def public_last(self):
        out = np.zeros(self.batch, dtype=np.uint32)
        check(_lib.load().zk_batch_public_last(self._h, _ptr(out)))
        return out

    def merkle_nodes(self, tree, first=0, count=None, coset_steps=0):
        """Nodes of batch tree `tree`: a heap over batch * m_l leaves whose node 2^log_batch - 1 + p roots proof p's tree.
        coset_steps: what the last proof built the tree with (m_l = layer_size >> coset_steps leaves per proof).  The nodes above the
        per-proof roots belong to no proof: the call hashes them on the host from the roots."""
        m = ((1 << (self.log_n + self.log_blowup)) >> max(tree - 1, 0)) >> coset_steps
        return _read_nodes(_lib.load().zk_batch_merkle_nodes, self._h, tree, 2 * m * self.batch - 1, first, count)

    def prove_raw(self):
        """Returns (proof bytes [batch][len] as a uint8 array, states [batch][32])."""
        plen = self.proof_len
        data = np.zeros((self.batch, plen), dtype=np.uint8)
        states = np.zeros((self.batch, 32), dtype=np.uint8)
        check(_lib.load().zk_batch_prove(self._h, data.ctypes.data_as(C.c_void_p), plen, states.ctypes.data_as(C.c_void_p)))
        return data, states

    def prove(self):
        data, states = self.prove_raw()
        last = self.public_last()
        return [Proof(states[p].tobytes(), data[p].tobytes(), self.log_n, self.log_blowup, int(last[p]), self.hash, self.queries,
                      self.grind_bits, self.fold_log, self.coset_leaves, self.stop_log, self.cap_log, self.ext_log) for p in range(self.batch)]

    def prove_shared(self):
        """zk_batch_prove_shared: ONE SharedProof of the batch's resident traces with the current settings."""
        plen = _proof_data_len(self, self.log_batch, self.shared_rows)
        data = np.zeros(max(plen, 1), dtype=np.uint8)
        state = np.zeros(32, dtype=np.uint8)
        got = C.c_size_t()
        check(_lib.load().zk_batch_prove_shared(self._h, _ptr(data), plen, C.byref(got), _ptr(state)))
        return SharedProof(state.tobytes(), data[:got.value].tobytes(), self.log_n, self.log_blowup, self.log_batch, self.public_last(), self.hash,
                           self.queries, self.grind_bits, self.fold_log, self.coset_leaves, self.stop_log, self.cap_log, self.shared_rows)


_ERR_VERIFY = -6


class SharedProof:
    """ONE proof of the 2^log_batch statements of a batch (BatchContext.prove_shared, zk_batch_prove_shared): the f trees are committed
    together, one FRI runs over the sum of the composition polynomials.  public_last: one value per statement.  shared_rows: the f values
    are committed as row leaves (BatchContext(shared_rows=True)) and the proof is checked by zk_verify_shared_rows."""

    def __init__(self, state, data, log_n, log_blowup, log_batch, public_last, hash="sha256", queries=1, grind_bits=0, fold_log=1,
                 coset_leaves=False, stop_log=0, cap_log=0, shared_rows=False):
        self.state, self.data = bytes(state), bytes(data)
        self.log_n, self.log_blowup, self.log_batch = log_n, log_blowup, log_batch
        self.public_last = _u32arr(public_last)
        self.hash, self.queries, self.grind_bits, self.fold_log = hash, queries, grind_bits, fold_log
        self.coset_leaves, self.stop_log, self.cap_log = bool(coset_leaves), stop_log, cap_log
        self.shared_rows = bool(shared_rows)

    def expected_len(self):
        """The length the format gives a shared proof of this shape."""
        return _proof_data_len(self, self.log_batch, self.shared_rows)

    def _verify(self, strict, out):
        if len(self.public_last) != 1 << self.log_batch:
            raise ZkError(-1, f"expected {1 << self.log_batch} public_last values")
        if self.shared_rows:
            return _lib.load().zk_verify_shared_rows(self.data, len(self.data), self.state if strict else None, self.log_n, self.log_blowup,
                                                     _ptr(self.public_last), self.log_batch, HASHES[self.hash], self.queries, self.grind_bits,
                                                     self.fold_log, int(self.coset_leaves), self.stop_log, self.cap_log, 1, C.byref(out))
        return _lib.load().zk_verify_shared(self.data, len(self.data), self.state if strict else None, self.log_n, self.log_blowup,
                                            _ptr(self.public_last), self.log_batch, HASHES[self.hash], self.queries, self.grind_bits,
                                            self.fold_log, int(self.coset_leaves), self.stop_log, self.cap_log, C.byref(out))

    def verify(self, strict=False):
        """Raises ZkError for a rejected proof; strict=True replays the channel first."""
        check(self._verify(strict, C.c_int32()))

    def check(self, strict=False):
        """The number of the check zk_verify_shared stops at: 0 = accepted.  Never raises for a rejected proof."""
        out = C.c_int32()
        rc = self._verify(strict, out)
        if rc not in (_lib.ZK_OK, _ERR_VERIFY) and not out.value:
            check(rc)
        return out.value


class Verifier:
    """Many proofs of one size checked at once on the GPU (zk_verifier_*).  Every result is the number Proof.check gives for
    that proof: 0 = accepted, otherwise the CPU verifier's check number."""

    def __init__(self, log_n, log_blowup, device=0, hash="sha256", queries=1, grind_bits=0, fold_log=1, coset_leaves=False, stop_log=0,
                 cap_log=0, log_batch=0, shared_rows=False, ext_log=0):
        """ext_log: 1 = the proofs have their challenges, cp and FRI layers in the quadratic extension E (zk_verifier_set_ext;
        Context(ext_log=1)); not with log_batch.
        log_batch, shared_rows: the proofs are shared proofs of 2^log_batch statements each (BatchContext.prove_shared), with row leaves
        when shared_rows (zk_verifier_set_shared; 0: plain proofs).
        cap_log: the proofs commit every tree by 2^cap_log digests (zk_verifier_set_merkle_cap; Context(cap_log=)).
        fold_log: the FRI folding factor 2^fold_log of the proofs to check (zk_verifier_set_fold; 1 = the reference).
        coset_leaves: the proofs were made with coset leaves (zk_verifier_set_coset_leaves; Context(coset_leaves=True)).
        stop_log: the proofs stop FRI early at a polynomial of 2^stop_log coefficients (zk_verifier_set_fri_stop; Context(stop_log=))."""
        _no_blake2s("Verifier", hash)
        self.log_n, self.log_blowup, self.hash, self.queries, self.grind_bits = log_n, log_blowup, hash, queries, grind_bits
        self.fold_log = 1
        self.coset_leaves = False
        self.stop_log = 0
        self.cap_log = 0
        self.log_batch, self.shared_rows = 0, False
        self.ext_log = 0
        self._h = C.c_void_p()
        check(_lib.load().zk_verifier_create(device, log_n, log_blowup, C.byref(self._h)))
        if hash != "sha256":
            check(_lib.load().zk_verifier_set_hash(self._h, HASHES.get(hash, -1)))   # an unknown name: ZK_ERR_INVALID
        if queries != 1:
            check(_lib.load().zk_verifier_set_queries(self._h, queries))
        if grind_bits:
            check(_lib.load().zk_verifier_set_grinding(self._h, grind_bits))
        if fold_log != 1:
            self.set_fold(fold_log)
        if coset_leaves:
            self.set_coset_leaves(True)
        if stop_log:
            self.set_fri_stop(stop_log)
        if cap_log:
            self.set_merkle_cap(cap_log)
        if log_batch or shared_rows:
            self.set_shared(log_batch, shared_rows)
        if ext_log:
            self.set_ext(ext_log)

    def set_ext(self, ext_log):
        """zk_verifier_set_ext: from the next run on, check proofs over E = F_P[u] / (u^2 - 5) (1) or base-field proofs (0).  ZkError, and
        the setting unchanged, for ext_log > 1 and for ext_log = 1 on a verifier of shared proofs."""
        check(_lib.load().zk_verifier_set_ext(self._h, ext_log))
        self.ext_log = ext_log

    def set_shared(self, log_batch, rows=False):
        """zk_verifier_set_shared: from the next run on, check shared proofs of 2^log_batch statements each (0: plain proofs), committed
        as row leaves when rows.  public_last is then 2^log_batch values per proof.  ZkError, and the setting unchanged, for
        log_batch >= 1 on a verifier with ext on."""
        check(_lib.load().zk_verifier_set_shared(self._h, log_batch, int(bool(rows))))
        self.log_batch, self.shared_rows = log_batch, bool(rows)

    def set_merkle_cap(self, cap_log):
        """zk_verifier_set_merkle_cap: from the next run on, check proofs whose trees are committed by 2^cap_log digests (0: by roots)."""
        check(_lib.load().zk_verifier_set_merkle_cap(self._h, cap_log))
        self.cap_log = cap_log

    def set_fri_stop(self, stop_log):
        """zk_verifier_set_fri_stop: from the next run on, check proofs that send the final polynomial's 2^stop_log coefficients
        (0: proofs folded down to a constant)."""
        check(_lib.load().zk_verifier_set_fri_stop(self._h, stop_log))
        self.stop_log = stop_log

    def set_fold(self, fold_log):
        """zk_verifier_set_fold: check proofs folded by 2^fold_log (1..3) between commitments from the next run on."""
        check(_lib.load().zk_verifier_set_fold(self._h, fold_log))
        self.fold_log = fold_log

    def set_coset_leaves(self, on=True):
        """zk_verifier_set_coset_leaves: from the next run on, check proofs with one coset per leaf and one path per group."""
        check(_lib.load().zk_verifier_set_coset_leaves(self._h, int(bool(on))))
        self.coset_leaves = bool(on)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().zk_verifier_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    @property
    def proof_len(self):
        return _proof_data_len(self, self.log_batch, self.shared_rows)

    def verify_raw(self, data, public_last, states=None):
        """data: [count, stride] uint8 (stride >= proof_len; BatchContext.prove_raw()'s array as it is), public_last: [count], or for
        shared proofs [count, 2^log_batch] (or flat, statement-major per proof), states: [count, 32] uint8 or None (not strict).
        Returns the check numbers as an int32 array of length count."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if data.ndim != 2:
            raise ZkError(-1, "verify_raw: data must be [count, stride]")
        count, stride = data.shape
        last = _u32arr(np.asarray(public_last).reshape(-1))
        if len(last) != count << self.log_batch:
            raise ZkError(-1, f"verify_raw: {len(last)} public_last values for {count} proofs of {1 << self.log_batch} statement(s)")
        st = None
        if states is not None:
            st = np.ascontiguousarray(states, dtype=np.uint8)
            if st.shape != (count, 32):
                raise ZkError(-1, f"verify_raw: states must be [{count}, 32]")
        out = np.zeros(count, dtype=np.int32)
        rc = _lib.load().zk_verifier_run(self._h, _ptr(data), stride, count, _ptr(st) if st is not None else None, _ptr(last), _ptr(out))
        if rc not in (_lib.ZK_OK, _ERR_VERIFY):
            check(rc)
        return out

    def verify(self, proofs, strict=True):
        """proofs: a list of Proof of this verifier's size, folding factor, leaf format and early stop (their data, state and public_last
        are used); with log_batch > 0 a list of SharedProof of 2^log_batch statements each."""
        proofs = list(proofs)
        plen = self.proof_len
        data = np.zeros((len(proofs), plen), dtype=np.uint8)
        for i, p in enumerate(proofs):
            if getattr(p, "fold_log", 1) != self.fold_log:
                raise ZkError(-1, f"verify: proof {i} was folded with fold_log {getattr(p, 'fold_log', 1)}, this verifier is set to {self.fold_log}")
            if bool(getattr(p, "coset_leaves", False)) != self.coset_leaves:
                names = {True: "coset leaves", False: "one-value leaves"}
                raise ZkError(-1, f"verify: proof {i} was made with {names[bool(getattr(p, 'coset_leaves', False))]}, "
                                  f"this verifier is set to {names[self.coset_leaves]}")
            if getattr(p, "stop_log", 0) != self.stop_log:
                raise ZkError(-1, f"verify: proof {i} was made with stop_log {getattr(p, 'stop_log', 0)}, this verifier is set to stop_log {self.stop_log}")
            if getattr(p, "cap_log", 0) != self.cap_log:
                raise ZkError(-1, f"verify: proof {i} was made with cap_log {getattr(p, 'cap_log', 0)}, this verifier is set to cap_log {self.cap_log}")
            if getattr(p, "log_batch", 0) != self.log_batch:
                raise ZkError(-1, f"verify: proof {i} was made with log_batch {getattr(p, 'log_batch', 0)}, this verifier is set to log_batch {self.log_batch}")
            if bool(getattr(p, "shared_rows", False)) != self.shared_rows:
                raise ZkError(-1, f"verify: proof {i} was made with shared_rows {bool(getattr(p, 'shared_rows', False))}, "
                                  f"this verifier is set to shared_rows {self.shared_rows}")
            if getattr(p, "ext_log", 0) != self.ext_log:
                raise ZkError(-1, f"verify: proof {i} was made with ext_log {getattr(p, 'ext_log', 0)}, this verifier is set to ext_log {self.ext_log}")
            if len(p.data) != plen:
                raise ZkError(-1, f"verify: proof {i} has {len(p.data)} bytes, this verifier takes {plen}")
            data[i] = np.frombuffer(p.data, dtype=np.uint8)
        if self.log_batch:
            last = np.array([np.asarray(p.public_last, dtype=np.uint32) for p in proofs], dtype=np.uint32).reshape(len(proofs), -1)
        else:
            last = np.array([p.public_last & 0xFFFFFFFF for p in proofs], dtype=np.uint32)
        states = np.array([np.frombuffer(p.state, dtype=np.uint8) for p in proofs], dtype=np.uint8).reshape(len(proofs), 32) if strict else None
        return self.verify_raw(data, last, states)


def shard_plan(world, log_n, log_blowup, min_layer_log=0, min_chunk_log=0, overlap_min_log=0, force_collectives=False, plain_collectives=False,
               exchange_cp=False, peer_copy=False):
    """zk_shard_plan: the layout zk_shard_create would choose (no GPU needed); a dict of the zk_shard_plan_info fields."""
    opt = _lib.ShardOptions(min_layer_log, min_chunk_log, overlap_min_log, int(force_collectives), 0, int(plain_collectives), 0, 0, int(exchange_cp), 0.0,
                            int(peer_copy))
    pl = _lib.ShardPlan()
    check(_lib.load().zk_shard_plan(world, log_n, log_blowup, C.byref(opt), C.byref(pl)))
    d = {k: v for k, v in pl.fields().items() if k != "piece_log"}
    d["piece_log"] = list(pl.piece_log)[:pl.sharded_layers + 1]
    return d


def shard_unique_id():
    """ncclGetUniqueId (rank 0): the 128 bytes every rank hands to ShardContext."""
    buf = C.create_string_buffer(128)
    check(_lib.load().zk_shard_unique_id(buf))
    return buf.raw


class ShardContext:
    """One proof sharded over `world` GPUs (zk_shard_*): this process is rank `rank`.  Collective: every rank
    constructs it and calls the same methods in the same order.  transport=None uses RCCL (native, inside the
    library) with the shared `unique_id`; a _lib.ShardTransport supplies the caller's own collectives."""

    def __init__(self, log_n, log_blowup, rank, world, unique_id=None, device=0, transport=None, min_layer_log=0, min_chunk_log=0,
                 overlap_min_log=0, force_collectives=False, no_root_board=False, hash="sha256", queries=1, plain_collectives=False,
                 single_build_stream=False, single_communicator=False, timeout_s=0.0, exchange_cp=False, peer_copy=False):
        _no_blake2s("ShardContext", hash)
        self.log_n, self.log_blowup, self.rank, self.world = log_n, log_blowup, rank, world
        self.hash, self.queries = hash, queries
        self._transport = transport                      # keeps the callbacks alive
        opt = _lib.ShardOptions(min_layer_log, min_chunk_log, overlap_min_log, int(force_collectives), int(no_root_board),
                                int(plain_collectives), int(single_build_stream), int(single_communicator), int(exchange_cp), float(timeout_s),
                                int(peer_copy))
        self._h = C.c_void_p()
        idb = C.create_string_buffer(bytes(unique_id), 128) if unique_id is not None else None
        check(_lib.load().zk_shard_create(device, rank, world, idb, C.byref(transport) if transport is not None else None,
                                          C.byref(opt), log_n, log_blowup, C.byref(self._h)))
        if hash != "sha256":
            check(_lib.load().zk_shard_set_hash(self._h, HASHES[hash]))
        if queries != 1:
            check(_lib.load().zk_shard_set_queries(self._h, queries))

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().zk_shard_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def trace_upload(self, trace):
        t = _u32arr(trace)
        check(_lib.load().zk_shard_trace_upload(self._h, _ptr(t), len(t)))

    def prove(self):
        cap = _lib.load().zk_proof_data_len_queries(self.log_n, self.log_blowup, self.queries)
        buf, st, n = C.create_string_buffer(cap), C.create_string_buffer(32), C.c_size_t()
        check(_lib.load().zk_shard_prove(self._h, buf, cap, C.byref(n), st))
        return Proof(st.raw, buf.raw[:n.value], self.log_n, self.log_blowup, self.last_transcript().public_last, self.hash, self.queries)

    def inject_failure(self, code=-4):
        """Test hook (zk_shard_inject_failure): this rank leaves the protocol with an error; peers must not hang."""
        return _lib.load().zk_shard_inject_failure(self._h, code)

    def self_test(self):
        """zk_shard_self_test: known-pattern all-to-all + all-gather through the transport (collective)."""
        check(_lib.load().zk_shard_self_test(self._h))

    def set_profiling(self, on):
        """zk_shard_set_profiling: HIP events around the exchanges of later proofs (stats(): exchange_ms, ...)."""
        check(_lib.load().zk_shard_set_profiling(self._h, int(bool(on))))

    def prove_channel(self, channel):
        check(_lib.load().zk_shard_prove_channel(self._h, channel._h))
        return channel.finalize(self.log_n, self.log_blowup, self.last_transcript().public_last)

    def lde_commit(self):
        out = C.create_string_buffer(32)
        check(_lib.load().zk_shard_lde_commit(self._h, out))
        return out.raw

    def last_transcript(self):
        info = _lib.TranscriptInfo()
        check(_lib.load().zk_shard_last_transcript(self._h, C.byref(info)))
        return info

    def layer_read(self, layer, offset, count):
        out = np.zeros(count, dtype=np.uint32)
        check(_lib.load().zk_shard_layer_read(self._h, layer, offset, count, _ptr(out)))
        return out

    def stats(self):
        st = _lib.ShardStats()
        check(_lib.load().zk_shard_get_stats(self._h, C.byref(st)))
        return st.fields()


def _generate_proof_coset(channel, ctx, a0, a1):
    """generate_proof with coset leaves (zk_ctx_set_coset_leaves), stage by stage: the tree over a group's input layer has that
    group's cosets as leaves; per query three f tuples, then per group the slots of one leaf and one path."""
    n, B, N, R, K = ctx.n, ctx.B, ctx.N, ctx.rounds, ctx.fold_log
    groups = [(r0, min(K, R - r0)) for r0 in range(0, R, K)]
    a = trace_fibsq(n - 1, a0, a1)
    ctx.trace_upload(a)
    ctx.lde()
    channel.commit(ctx.merkle_commit(0))
    ctx.compose([channel.get_u32() for _ in range(3)])
    channel.commit(ctx.merkle_commit(1, groups[0][1]))
    for j, (r0, steps) in enumerate(groups):
        ctx.fri_fold_multi(r0, steps, channel.get_u32())
        channel.commit(ctx.merkle_commit(1 + r0 + steps, groups[j + 1][1] if j + 1 < len(groups) else 0))
    last = ctx.layer_read(1 + R)
    if not (last == last[0]).all():
        raise ZkError(-7, "last FRI layer is not constant")
    channel.commit(int(last[0]))
    if ctx.grind_bits:
        raise ZkError(-1, "generate_proof: grinding is part of Context.prove(), not of the stage-by-stage flow")
    xs = [channel.get_u32() % (N - 2 * B) for _ in range(ctx.queries)]
    for x in xs:
        for idx in (x, x + B, x + 2 * B):
            channel.commit((int(ctx.layer_read(0, idx, 1)[0]), ctx.merkle_path(0, idx)))
        for r0, steps in groups:
            leaves = (N >> r0) >> steps
            c = x % leaves
            channel.commit(tuple(int(ctx.layer_read(1 + r0, c + u * leaves, 1)[0]) for u in range(1 << steps)) + (ctx.merkle_path(1 + r0, c),))
    proof = channel.finalize(ctx.log_n, ctx.log_blowup, int(a[n - 2]))
    proof.hash, proof.queries, proof.fold_log, proof.coset_leaves = ctx.hash, ctx.queries, K, True
    return proof


def generate_proof(channel, log_n=10, log_blowup=3, a0=1, a1=3141592, ctx=None):
    """prover.rs:9-293, stage by stage over the C ABI, driven by `channel`.

    The reference literals are the defaults (trace 1023 values, domain 8192).
    Context.prove() is the same flow inside one C call.  A context with coset leaves on (Context(coset_leaves=True)) gives the
    coset-leaf proof of its folding factor, through the same stage calls.
    """
    own = ctx is None
    ctx = ctx or Context(log_n, log_blowup)
    try:
        if ctx.coset_leaves:
            return _generate_proof_coset(channel, ctx, a0, a1)
        n, B, N, R = ctx.n, ctx.B, ctx.N, ctx.rounds
        a = trace_fibsq(n - 1, a0, a1)                       # prover.rs:32-39
        ctx.trace_upload(a)
        ctx.lde()                                            # prover.rs:60-70
        channel.commit(ctx.merkle_commit(0))                 # prover.rs:81-85
        alphas = [channel.get_u32() for _ in range(3)]       # prover.rs:163-165
        ctx.compose(alphas)                                  # prover.rs:166-173
        channel.commit(ctx.merkle_commit(1))                 # prover.rs:176-180
        for r in range(R):                                   # prover.rs:198-225
            beta = channel.get_u32()
            ctx.fri_fold(r, beta)
            channel.commit(ctx.merkle_commit(2 + r))
        last = ctx.layer_read(1 + R)
        if not (last == last[0]).all():                      # prover.rs:238
            raise ZkError(-7, "last FRI layer is not constant")
        channel.commit(int(last[0]))                         # prover.rs:254
        x = channel.get_u32() % (N - 2 * B)                  # prover.rs:263
        for layer, idx in ((0, x), (0, x + B), (0, x + 2 * B), (1, x)):      # prover.rs:266-277
            channel.commit((int(ctx.layer_read(layer, idx, 1)[0]), ctx.merkle_path(layer, idx)))
        for i in range(R):                                   # prover.rs:280-289
            ln = N >> i
            xi = x % ln
            nx = (xi + ln // 2) % ln
            channel.commit((int(ctx.layer_read(1 + i, xi, 1)[0]), int(ctx.layer_read(1 + i, nx, 1)[0]),
                            ctx.merkle_path(1 + i, xi), ctx.merkle_path(1 + i, nx)))
        return channel.finalize(log_n, log_blowup, int(a[n - 2]))   # prover.rs:292
    finally:
        if own:
            ctx.close()
