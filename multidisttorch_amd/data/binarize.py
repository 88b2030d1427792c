"""``--binarize``: Bernoulli-resampled (or thresholded) data on the device.

BCE against a grey level is not the negative log of a normalised likelihood;
against a {0, 1} pixel it is. A ``Binarizer`` owns a compact ``[n, D]`` float32
buffer of {0, 1} for the rows ``X[idx]`` of one split and rewrites it IN PLACE
(``refresh``), so a trainer bound to ``.data`` / ``.index()`` keeps its bound
pointer and every captured step graph stays valid across epochs.

Modes (csrc/kernels/binarize.h has the Philox counter layout):
  threshold   ``x >= 0.5``, no RNG, written once
  static      one Bernoulli draw for the whole trial (epoch key 0), written once
  dynamic     a fresh draw per epoch (the epoch number is the key, so a resumed
              trial redraws exactly what an uninterrupted one would)
A test split (``split = 1``) is always drawn once with epoch key 0: the fixed
binarized test set. Draws are keyed by the global data-set row, so replicas of
a data-parallel group produce the same bits without communicating.

On a GPU tensor the rewrite is one launch of ``_C.binarize_rows`` on the
current stream; elsewhere it is the numpy oracle ``ops.philox.bernoulli_rows``
(bit-identical).
"""

from __future__ import annotations

import torch

from ..ops import native
from ..ops.philox import BINARIZE_MODES, bernoulli_rows

__all__ = ["Binarizer", "BINARIZE_CHOICES", "check_mode"]

BINARIZE_CHOICES = ("none",) + BINARIZE_MODES


def check_mode(mode: str, allow_none: bool = True) -> str:
    """``mode`` if it names a binarization (or ``none``); ValueError otherwise."""
    ok = BINARIZE_CHOICES if allow_none else BINARIZE_MODES
    if mode not in ok:
        raise ValueError(f"unknown binarize mode {mode!r} (one of {', '.join(ok)})")
    return mode


class Binarizer:
    def __init__(self, mode: str, seed: int, X: torch.Tensor, idx: torch.Tensor, split: int):
        self.mode = check_mode(mode, allow_none=False)
        if split not in (0, 1):
            raise ValueError("split must be 0 (train) or 1 (test)")
        if X.dtype != torch.float32 or X.dim() != 2 or X.shape[1] < 1:
            raise ValueError("X must be a float32 [N, D] tensor")
        self.seed, self.split = int(seed), int(split)
        self.X = X.contiguous()
        self.idx = idx.to(device=X.device, dtype=torch.int32).contiguous().view(-1)
        n = self.idx.numel()
        if n and (int(self.idx.min()) < 0 or int(self.idx.max()) >= X.shape[0]):
            raise IndexError("row index outside the data set")
        if X.is_cuda:  # a GPU split needs the kernel: no host fall-back
            native.require().binarize_check(n, X.shape[1], X.shape[0], self.mode, self.split)
        self.data = torch.zeros(n, X.shape[1], dtype=torch.float32, device=X.device)
        self._index = torch.arange(n, dtype=torch.int32, device=X.device)
        self.epoch_key = None  # the epoch word of the draw the buffer holds; None = not yet written

    def __len__(self):
        return self.data.shape[0]

    def index(self) -> torch.Tensor:
        """``arange(n)``: the index list to bind ``.data`` with."""
        return self._index

    def key_for(self, epoch: int) -> int:
        """The epoch counter word of ``refresh(epoch)``."""
        return int(epoch) if self.mode == "dynamic" and self.split == 0 else 0

    def refresh(self, epoch: int = 0) -> bool:
        """Make the buffer hold the rows of ``epoch``, rewriting it in place on
        the current stream when it does not already; True if it was rewritten
        (the caller then tells the trainer: ``train_data_changed()``)."""
        key = self.key_for(epoch)
        if self.epoch_key == key:
            return False
        if self.X.is_cuda:
            native.require().binarize_rows(self.X, self.idx, self.data, self.seed, key, self.split, self.mode)
        else:
            out = bernoulli_rows(self.X.numpy(), self.idx.numpy(), self.seed, key, self.split, self.mode)
            self.data.copy_(torch.from_numpy(out))
        self.epoch_key = key
        return True
