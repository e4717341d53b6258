"""What the per-element GPU tests of the C ABI share (tests/test_gpu_heads.py, tests/test_gpu_rows.py): pointer arguments and output
buffers pre-filled with NaN sentinels, with pad rows behind them."""
import ctypes as C

import torch

SENT16 = 0x7FC1                      # bf16 NaN payload no kernel writes (as tests/test_gpu_gemm_exact.py)
SENT32 = 0x7FC01234                  # fp32 NaN payload
PAD_ROWS = 8


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(t):
    return None if t is None else t.cuda()


class Out:
    """[rows, cols] output of `dtype` filled with the NaN sentinel, PAD_ROWS more rows behind it; `init` (a CPU tensor) pre-fills the body."""

    def __init__(self, rows, cols, dtype, init=None):
        self.rows, self.cols, self.dtype = rows, cols, dtype
        n = (rows + PAD_ROWS) * cols
        if dtype == torch.bfloat16:
            self.buf = torch.full((n,), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        elif dtype == torch.float32:
            self.buf = torch.full((n,), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
        else:
            self.buf = torch.full((n,), -7, dtype=dtype, device="cuda")
        if init is not None:
            self.buf[:rows * cols] = init.reshape(-1).to(self.buf.device)

    def _intact(self, part):
        if self.dtype == torch.bfloat16:
            return bool((part.view(torch.int16) == SENT16).all())
        if self.dtype == torch.float32:
            return bool((part.view(torch.int32) == SENT32).all())
        return bool((part == -7).all())

    def body(self):
        """The body on the CPU, after checking that nothing was written behind it."""
        torch.cuda.synchronize()
        assert self._intact(self.buf[self.rows * self.cols:]), f"wrote behind the {self.rows} x {self.cols} output"
        return self.buf[:self.rows * self.cols].view(self.rows, self.cols).cpu()

    def untouched(self):
        torch.cuda.synchronize()
        return self._intact(self.buf)
