"""What "uint8 RGB frames on the GPU" means to the pixel-side modules (jpeg, png, color, motion, video_io): one argument contract and the small host helpers the
encoders share.  Pure Python and torch; no library is loaded here.  A module keeps what is its own (JPEG's 65535, colour's 2^31, motion's pairs, PNG's geometry)
next to its call of `check_frames`; every refusal comes before any kernel call, and `check_device` comes last, so that a wrong argument is named with or without a
device."""
import torch


def is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def check_frames(frames, who, dims=(4, 5)):
    """The shape contract of every entry point, checked before any kernel call."""
    if not isinstance(frames, torch.Tensor):
        raise ValueError(f"{who}: expected a tensor of frames")
    if frames.dtype != torch.uint8:
        raise NotImplementedError(f"{who}: uint8 frames only (video_io's \"uint8\" output), got {frames.dtype}")
    want = " or ".join({3: "[H, W, 3]", 4: "[F, H, W, 3]", 5: "[B, T, H, W, 3]"}[d] for d in dims)
    if frames.dim() not in dims or frames.shape[-1] != 3 or frames.numel() < 1:
        raise ValueError(f"{who}: expected {want} (RGB, three channels) with at least one pixel, got {tuple(frames.shape)}")


def check_device(frames, who):
    """after every other check, so that a wrong argument is named with or without a device"""
    if not frames.is_cuda:
        raise RuntimeError(f"{who}: expected a GPU tensor (tokensgen_amd has no CPU path)")


def gpu_device(device, who):
    """`device` (None: the current GPU) as a torch.device with its index; RuntimeError where it is no GPU"""
    dev = torch.device(device) if device is not None else None
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{who}: needs a GPU (tokensgen_amd has no CPU path)")
        return torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: needs a GPU device, got {dev} (tokensgen_amd has no CPU path)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None and torch.cuda.is_available() else dev


def single_frame(frame, who):
    """One frame per file: checked [H, W, 3] or [1, H, W, 3] -> [1, H, W, 3] (a view)."""
    if frame.dim() == 4 and frame.shape[0] != 1:
        raise ValueError(f"{who}: one frame per file, got {frame.shape[0]}")
    return frame.reshape(1, *frame.shape[-3:])


def split_bytes(data, offsets):
    """What an encoder returns (data uint8 [n] on the device, offsets int64 [F + 1] on the host), copied to the host and cut: a list of one `bytes` per frame."""
    host, o = data.cpu().numpy().tobytes(), offsets.tolist()
    return [host[o[i]:o[i + 1]] for i in range(len(o) - 1)]
