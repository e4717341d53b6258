"""Time the dh + GEGLU' launch (down-projection dgrad with the gated-GELU backward in its epilogue) of the C1 step, A/B over
gget_debug_set(L.KEY_GEMM_VARIANT, bits): L.GEMM_ONE_BLOCK_PER_CU (32) = one workgroup per CU instead of two.  GGET_T = rows (default 5696)."""
import ctypes as C, importlib, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
L = importlib.import_module("graph-gpt_amd._lib"); lib = L.load()
menu0 = L.debug_get(L.KEY_GEMM_VARIANT)   # (restored at the end)
P = lambda t: C.c_void_p(t.data_ptr()); st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
d, ff = 768, 3072
for T in [int(x) for x in os.environ.get("GGET_T", "5696,8192").split(",")]:
    dy = torch.randn(T, d, device="cuda").to(torch.bfloat16); w = (torch.randn(d, ff, device="cuda") * 0.02).to(torch.bfloat16)
    gu = torch.randn(T, 2 * ff, device="cuda").to(torch.bfloat16); dgu = torch.empty_like(gu)
    dh = torch.empty(T, ff, dtype=torch.bfloat16, device="cuda")
    flush = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    for rnd in range(3):
        for bits in [int(x) for x in os.environ.get('GGET_BITS', '0,32').split(',')]:
            L.check(lib.gget_debug_set(L.KEY_GEMM_VARIANT, bits))
            ts = []
            for it in range(12):
                flush.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                L.check(lib.gget_op_down_dgrad_geglu(P(dy), P(w), P(gu), P(dgu), P(dh), T, d, ff, st))
                e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            ts = sorted(ts[2:])
            print(f"T={T} variant={bits:2d}: median {ts[len(ts)//2]:7.1f} us  min {ts[0]:7.1f} us", flush=True)
    L.check(lib.gget_debug_set(L.KEY_GEMM_VARIANT, menu0))