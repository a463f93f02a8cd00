"""zk_verifier_set_ext without a GPU: the null-handle answers of the C ABI, the declarations of header, ctypes table and Rust binding under
an unchanged ABI version, and the Python Verifier's arguments (a Verifier itself needs a device: tests/test_gpu_verify_ext.py)."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zk_verifier_set_ext", "zk_verifier_get_ext")


def test_null_handle(zk):
    lib = zk.load()
    for ext_log in (0, 1, 2):
        assert lib.zk_verifier_set_ext(None, ext_log) == -1          # ZK_ERR_INVALID
    assert b"null verifier" in lib.zk_last_error()
    assert lib.zk_verifier_get_ext(None) == 0


def test_declared_in_header_ctypes_and_rust(zk):
    header = open(os.path.join(ROOT, "include", "zkstark_amd.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "zkstark_amd_sys.rs")).read()
    assert re.search(r"int zk_verifier_set_ext\(zk_verifier \*v, uint32_t ext_log\);", header)
    assert re.search(r"uint32_t zk_verifier_get_ext\(const zk_verifier \*v\);", header)
    assert "pub fn zk_verifier_set_ext(v: *mut zk_verifier, ext_log: u32) -> c_int;" in rust
    assert "pub fn zk_verifier_get_ext(v: *const zk_verifier) -> u32;" in rust
    for name in NAMES:
        assert name in zk._lib.SYMBOLS, name
    assert re.search(r"#define ZK_ABI_VERSION 6u", header)           # functions only: the ABI version stays
    assert zk.load().zk_abi_version() == zk._lib.ABI_VERSION == 6


def test_verifier_takes_ext_log(zk):
    init = inspect.signature(zk.Verifier.__init__).parameters
    assert init["ext_log"].default == 0
    assert list(inspect.signature(zk.Verifier.set_ext).parameters) == ["self", "ext_log"]
    src = inspect.getsource(zk.Verifier.verify)
    assert "ext_log" in src                                           # verify names an ext_log mismatch before any byte is read
