"""What the *_device functions of the commands share around a launch: uploads, the scratch an entry point sizes, the bit pattern
the tests put into buffers beforehand, the stream.  Imports torch: the commands import this module where they import torch."""
import numpy as np
import torch

from . import _lib


def put(v, dtype, device):
    """v as a C-contiguous array of `dtype` (None: its own), copied to the device."""
    return torch.from_numpy(np.ascontiguousarray(v, dtype=dtype)).to(device)


def fill_bits(fill):
    """A 32-bit pattern (tests: 0xFFFFFFFF, a NaN's bits) as the int32 that Tensor.fill_ takes."""
    return int(np.array(fill, dtype=np.uint32).view(np.int32))


def prefill(tensors, fill):
    """Tests: every 32-bit word of the tensors holds `fill` before a launch, in the order given.  fill None: nothing."""
    if fill is not None:
        for x in tensors:
            x.view(torch.int32).fill_(fill_bits(fill))


def work_buffer(lib, sizer_name, *args, device, fill=None):
    """(scratch tensor, work_bytes) for the launch whose sizer entry point is lib.<sizer_name>(*args): at least 16 bytes, so
    that there is a pointer to pass; a negative size is the sizer's refusal (loc_last_error says why)."""
    work_bytes = int(getattr(lib, sizer_name)(*args))
    if work_bytes < 0:
        _lib.check(-1, sizer_name)
    work = torch.empty(max(work_bytes // 4, 4), dtype=torch.float32, device=device)
    prefill((work,), fill)
    return work, work_bytes


def stream():
    """The current stream of the current device, as the entry points take it."""
    return torch.cuda.current_stream().cuda_stream
