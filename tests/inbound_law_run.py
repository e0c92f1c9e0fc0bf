"""Child process of tests/test_inbound_gpu.py: loads the test build of the library (SRG_LIB_PATH,
-DSRG_TEST_HOOKS), asks its test-only kernel for the control law's increments of the counts given
as a JSON list on the command line, and prints them as a JSON list."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shadow_amd import _native as N  # noqa: E402


def main():
    counts = json.loads(sys.argv[1])
    L = N.lib()
    f = L.srg_test_inbound_control_law
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(512)
    rc = L.srg_create(ctypes.byref(h), 0, err, len(err))
    assert rc == N.SRG_OK, err.value
    a = (ctypes.c_uint64 * len(counts))(*counts)
    out = (ctypes.c_uint64 * len(counts))()
    rc = f(h, a, len(counts), out)
    assert rc == N.SRG_OK, rc
    L.srg_destroy(h)
    print(json.dumps([int(x) for x in out]))


if __name__ == "__main__":
    main()
