"""zk_batch_set_merkle_cap / _get_merkle_cap / zk_batch_merkle_cap_log / zk_batch_merkle_cap without a GPU: declared in the header,
exported by the built library, named by the generated Rust file, their null-handle answers, and an ABI version that did not move (the
option is additive and off by default)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zk_batch_set_merkle_cap", "zk_batch_get_merkle_cap", "zk_batch_merkle_cap_log", "zk_batch_merkle_cap")


def test_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "zkstark_amd.h")).read()
    assert re.search(r"^int zk_batch_set_merkle_cap\(zk_batch \*b, uint32_t cap_log\);$", text, re.M)
    assert re.search(r"^uint32_t zk_batch_get_merkle_cap\(const zk_batch \*b\);$", text, re.M)
    assert re.search(r"^uint32_t zk_batch_merkle_cap_log\(const zk_batch \*b, uint32_t tree\);$", text, re.M)
    assert re.search(r"^int zk_batch_merkle_cap\(zk_batch \*b, uint32_t tree, size_t proof, uint8_t \*out, size_t out_len\);$", text, re.M)


def test_exported_by_the_library(zk):
    raw = C.CDLL(os.path.join(ROOT, "zkstark_amd", "libzkstark_amd.so"))
    for name in NAMES:
        assert getattr(raw, name) is not None                # AttributeError: the symbol is missing
        assert hasattr(zk.load(), name)


def test_named_by_the_rust_bindings():
    text = open(os.path.join(ROOT, "bindings", "rust", "zkstark_amd_sys.rs")).read()
    for name in NAMES:
        assert re.search(r"\bpub fn " + name + r"\(", text), name


def test_null_handle(zk):
    lib = zk.load()
    out = C.create_string_buffer(32)
    assert lib.zk_batch_set_merkle_cap(None, 4) == -1        # ZK_ERR_INVALID
    assert lib.zk_batch_set_merkle_cap(None, 0) == -1
    assert lib.zk_batch_merkle_cap(None, 0, 0, out, 32) == -1
    assert lib.zk_batch_get_merkle_cap(None) == 0
    assert lib.zk_batch_merkle_cap_log(None, 0) == 0


def test_python_takes_the_cap(zk):
    import inspect
    assert "cap_log" in inspect.signature(zk.BatchContext.__init__).parameters
    assert hasattr(zk.BatchContext, "set_merkle_cap") and hasattr(zk.BatchContext, "merkle_cap")


def test_abi_version_is_unchanged(zk):
    assert zk.load().zk_abi_version() == 6
