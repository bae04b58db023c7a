"""Host time of the two decode-level queries (hyd_decode_kv_quant_supported, hyd_decode_workspace_bytes) on one grouped-query fp8 shape:
a plain ctypes loop, no device needed.  HYDRAGEN_HIP_LIB picks the library, so two builds can be timed side by side.

    python tests/probes/decode_query_time_probe.py [calls] [repeats]      (profiles/suffix_plan.md)
"""
import ctypes as C
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

from hydragen_amd import _lib  # noqa: E402
from tests.abi_table import decode, kvq  # noqa: E402


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 300_000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    lib = _lib.load()
    d = decode(B=64, Hq=32, Hkv=8, kv_len=256, levels=((1, 4096), (8, 512)))   # a two-level decode step on grouped-query heads
    kq = kvq(flags=_lib.HYD_KVQ_GQA)
    dp, kp = C.byref(d), C.byref(kq)
    assert lib.hyd_decode_kv_quant_supported(dp, kp) == 1 and lib.hyd_decode_workspace_bytes(dp) > 0
    for name, call in (("hyd_decode_kv_quant_supported", lambda: lib.hyd_decode_kv_quant_supported(dp, kp)),
                       ("hyd_decode_workspace_bytes", lambda: lib.hyd_decode_workspace_bytes(dp))):
        ns = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            ns.append((time.perf_counter() - t0) / calls * 1e9)
        print(f"{name}: {' '.join(f'{x:.0f}' for x in ns)} ns per call ({calls} calls, ctypes overhead included)")


if __name__ == "__main__":
    main()
