"""zk_verifier_set_shared without a GPU: the null-handle answers of the C ABI, the declarations of header, ctypes table and Rust binding,
and the Python Verifier's arguments (a Verifier itself needs a device: tests/test_gpu_verify_shared.py)."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zk_verifier_set_shared", "zk_verifier_get_shared", "zk_verifier_get_shared_rows")


def test_null_handle(zk):
    lib = zk.load()
    assert lib.zk_verifier_set_shared(None, 1, 0) == -1
    assert lib.zk_verifier_set_shared(None, 0, 0) == -1 and lib.zk_verifier_set_shared(None, 3, 1) == -1
    assert lib.zk_verifier_get_shared(None) == 0
    assert lib.zk_verifier_get_shared_rows(None) == 0


def test_declared_in_header_ctypes_and_rust(zk):
    header = open(os.path.join(ROOT, "include", "zkstark_amd.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "zkstark_amd_sys.rs")).read()
    assert re.search(r"int zk_verifier_set_shared\(zk_verifier \*v, uint32_t log_batch, int row_leaves\);", header)
    assert re.search(r"uint32_t zk_verifier_get_shared\(const zk_verifier \*v\);", header)
    assert re.search(r"int zk_verifier_get_shared_rows\(const zk_verifier \*v\);", header)
    for name in NAMES:
        assert f"pub fn {name}(" in rust, name
        assert name in zk._lib.SYMBOLS, name
    assert zk.load().zk_abi_version() == zk._lib.ABI_VERSION      # functions only: the ABI version stays


def test_verifier_takes_the_shared_settings(zk):
    init = inspect.signature(zk.Verifier.__init__).parameters
    assert init["log_batch"].default == 0 and init["shared_rows"].default is False
    params = inspect.signature(zk.Verifier.set_shared).parameters
    assert list(params) == ["self", "log_batch", "rows"] and params["rows"].default is False
