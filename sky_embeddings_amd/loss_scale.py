"""Dynamic loss scale of an optimiser step whose loss is the CALLER's code (the downstream predictor in fp16: utils.vit).

The MIM engines plan a static scale from the number of masked elements, because their loss kernel is the library's.  A predictor's
loss is arbitrary torch code -- cross-entropy, MSE, uncertainty-weighted MSE on labels of any magnitude -- so nothing can be
planned: the gradients are probed on the device instead (``skyemb_grad_probe``: any +-inf / NaN, and the largest finite |g|), the
optimiser's launches skip themselves when the probe fired (``skyemb_adamw_guarded``), and the scale backs off and grows again with
``torch.amp.GradScaler``'s policy exactly:

* after a step whose flag was set: ``scale *= backoff_factor``, the growth tracker returns to 0;
* otherwise the tracker counts up; when it reaches ``growth_interval``: ``scale *= growth_factor``, tracker 0.

Scale and factors are powers of two, so scaling d loss / d predictions and dividing the scale out in the optimiser's
``grad_scale`` are exact.  ``dynamic=False`` keeps the scale where it is; the step is probed and skipped all the same.

One optimiser step costs one extra read of the gradients it consumes and ONE 8-byte device-to-host copy (``finish_step``).
"""
from __future__ import annotations

import math
import struct

import torch

from . import ops

_F32_MAX = float(torch.finfo(torch.float32).max)


def is_power_of_two(x) -> bool:
    try:
        x = float(x)
    except (TypeError, ValueError):
        return False
    return x > 0.0 and math.isfinite(x) and math.frexp(x)[0] == 0.5


class LossScaler:
    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, dynamic=True):
        assert is_power_of_two(init_scale), f"init_scale must be a power of two, got {init_scale!r}"
        assert is_power_of_two(growth_factor) and growth_factor > 1.0, f"growth_factor must be a power of two above 1, got {growth_factor!r}"
        assert is_power_of_two(backoff_factor) and backoff_factor < 1.0, f"backoff_factor must be a power of two below 1, got {backoff_factor!r}"
        assert int(growth_interval) >= 1, "growth_interval must be at least 1"
        self.scale = float(init_scale)
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval, self.dynamic = int(growth_interval), bool(dynamic)
        self.growth_tracker = 0
        self.skipped_steps = 0
        self.last_absmax = 0.0          # largest finite |gradient| of the last finished step, loss scale divided out
        self.last_overflow = False
        self.state = None               # device int32[2]: {overflow flag, fp32 bits of the largest finite |scaled gradient|}

    # ---- host policy (torch._amp_update_scale_) ---------------------------------------------------------------------------------
    def update(self, found_inf: bool):
        """The scale / tracker update after a step whose gradients did (found_inf) or did not overflow."""
        self.last_overflow = bool(found_inf)
        if found_inf:
            self.skipped_steps += 1
        if not self.dynamic:
            return
        if found_inf:
            self.scale *= self.backoff_factor
            self.growth_tracker = 0
            return
        self.growth_tracker += 1
        if self.growth_tracker == self.growth_interval:
            grown = self.scale * self.growth_factor
            if grown <= _F32_MAX:       # (torch: the scale stays put where the grown one would not be a finite fp32)
                self.scale = grown
            self.growth_tracker = 0

    # ---- device side ------------------------------------------------------------------------------------------------------------
    def to(self, device):
        if self.state is None or self.state.device != torch.device(device):
            self.state = torch.zeros(2, device=device, dtype=torch.int32)
        return self

    def begin_step(self):
        """Zeroes the two state words on the stream (a fill launch, not a copy): probes accumulate into them afterwards."""
        assert self.state is not None, "LossScaler.to(device) first (utils.vit.VisionTransformer does it)"
        self.state.zero_()

    def probe(self, g, n=None):
        ops.grad_probe(g, g.numel() if n is None else n, self.state)

    def finish_step(self) -> bool:
        """Reads both words (the step's one device-to-host copy), updates the scale; -> True if the step was APPLIED."""
        flag, bits = self.state.tolist()
        scale_used = self.scale
        self.last_absmax = struct.unpack("<f", struct.pack("<I", bits & 0xffffffff))[0] / scale_used
        self.update(flag != 0)
        return flag == 0

    # ---- checkpoints ------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"scale": self.scale, "growth_tracker": self.growth_tracker, "skipped_steps": self.skipped_steps}

    def load_state_dict(self, sd):
        assert is_power_of_two(sd["scale"]), f"loss scale must be a power of two, got {sd['scale']!r}"
        self.scale = float(sd["scale"])
        self.growth_tracker = int(sd.get("growth_tracker", 0))
        self.skipped_steps = int(sd.get("skipped_steps", 0))


def make_loss_scaler(spec):
    """'dynamic' | a power of two (fixed scale) | a LossScaler -> LossScaler."""
    if isinstance(spec, LossScaler):
        return spec
    if isinstance(spec, str) and spec.strip().lower() == "dynamic":
        return LossScaler()
    if isinstance(spec, str):
        try:
            spec = float(ast_number(spec))
        except ValueError:
            raise ValueError(f"loss_scale must be 'dynamic' or a power of two, got {spec!r}") from None
    if not is_power_of_two(spec):
        raise ValueError(f"loss_scale must be 'dynamic', a power of two or a LossScaler, got {spec!r}")
    return LossScaler(init_scale=float(spec), dynamic=False)


def ast_number(text):
    """'1024', '2**10', '65536.0' -> a number (ini values); ValueError otherwise."""
    import ast
    try:
        node = ast.parse(text.strip(), mode="eval").body
    except SyntaxError:
        raise ValueError(text) from None

    def ev(n):
        if isinstance(n, ast.Constant) and isinstance(n.value, (int, float)) and not isinstance(n.value, bool):
            return n.value
        if isinstance(n, ast.BinOp) and isinstance(n.op, ast.Pow):
            return ev(n.left) ** ev(n.right)
        raise ValueError(text)
    return ev(node)
