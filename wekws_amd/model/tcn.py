"""Trainable mirrors of the reference's TCN backbone (wekws/model/tcn.py) without the quantisation stubs: ``Block``,
``CnnBlock``, ``DsCnnBlock`` and ``TCN`` with the same constructors, state-dict keys and shapes and the same
``forward(x, in_cache) -> (out, cache)``, so state dicts go both ways (and into the packed inference model,
``wekws_amd.model.kws_model``).

The depthwise convolution of a ``DsCnnBlock`` is a ``wekws_amd.model.depthwise.DepthwiseConv1d``: with an empty cache it is
called with ``left_pad = padding``, so the block's ``F.pad`` copy is not made and, for float32 device tensors, the HIP kernels
run.  With a non-empty cache (streaming) the block does what the reference does: ``torch.cat``, then the
convolution.  The pointwise convolution of a ``DsCnnBlock`` is constructed as an ``nn.Conv1d`` and stays torch's unless
``wekws_amd.model.pointwise.use_device_pointwise_convs`` has swapped it for a ``PointwiseConv1d``.  The dense
convolution of a ``CnnBlock`` is constructed as an ``nn.Conv1d`` behind the block's ``F.pad`` and stays torch's unless
``wekws_amd.model.dense.use_device_dense_convs`` has swapped it for a ``DenseConv1d``: then it is called with
``left_pad`` and the ``F.pad`` copy is not made.  Dropout stays torch's; so do BatchNorm and ReLU unless
``wekws_amd.model.batchnorm.use_device_batchnorms`` has set a ``DsCnnBlock``'s ``fused_norm``: then each BatchNorm is a
``DeviceBatchNorm1d`` that is called with ``relu=True`` and the ReLU modules are skipped.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from wekws_amd.model.dense import DenseConv1d
from wekws_amd.model.depthwise import DepthwiseConv1d


def _empty_cache() -> torch.Tensor:
    return torch.zeros(0, 0, 0, dtype=torch.float)


def padded_tail(x: torch.Tensor, padding: int) -> torch.Tensor:
    """``F.pad(x, (padding, 0))[:, :, -padding:]`` -- the reference's new cache for an empty one -- without padding the whole
    tensor: the last ``padding`` columns of ``x``, with zeros in front where ``x`` is shorter."""
    T = x.size(2)
    if padding == 0:
        return x                                       # (the reference's slice [-0:] is the whole tensor)
    if T >= padding:
        return x[:, :, T - padding:]
    return F.pad(x, (padding - T, 0), value=0.0)


class Block(nn.Module):

    def __init__(self, channel: int, kernel_size: int, dilation: int, dropout: float = 0.1):
        super().__init__()
        self.padding = (kernel_size - 1) * dilation

    def _convolve(self, y: torch.Tensor, left_pad: int) -> torch.Tensor:
        """self.cnn (defined in the subclass) over ``y`` with ``left_pad`` zeros in front of every row."""
        raise NotImplementedError

    def forward(self, x: torch.Tensor, cache: torch.Tensor = _empty_cache()) -> Tuple[torch.Tensor, torch.Tensor]:
        """x (B, D, T); cache (B, D, self.padding) or empty -> (output (B, D, T), new cache (B, D, self.padding))."""
        if cache.size(0) == 0:
            new_cache = padded_tail(x, self.padding)
            y = self._convolve(x, self.padding)
        else:
            y = torch.cat((cache, x), dim=2)
            assert y.size(2) > self.padding
            new_cache = y[:, :, -self.padding:]
            y = self._convolve(y, 0)
        y = y + x  # residual connection
        return y, new_cache


class CnnBlock(Block):

    def __init__(self, channel: int, kernel_size: int, dilation: int, dropout: float = 0.1):
        super().__init__(channel, kernel_size, dilation, dropout)
        self.cnn = nn.Sequential(
            nn.Conv1d(channel, channel, kernel_size, stride=1, dilation=dilation),
            nn.BatchNorm1d(channel),
            nn.ReLU(),
            nn.Dropout(dropout),
        )

    def _convolve(self, y, left_pad):
        if isinstance(self.cnn[0], DenseConv1d):       # swapped by use_device_dense_convs: it supplies the padding's zeros itself
            y = self.cnn[0](y, left_pad)
            for layer in list(self.cnn)[1:]:
                y = layer(y)
            return y
        if left_pad:
            y = F.pad(y, (left_pad, 0), value=0.0)
        return self.cnn(y)


class DsCnnBlock(Block):
    """Depthwise separable convolution."""

    fused_norm = False      # set by use_device_batchnorms: cnn[1] and cnn[4] are DeviceBatchNorm1ds that apply the ReLUs behind them

    def __init__(self, channel: int, kernel_size: int, dilation: int, dropout: float = 0.1):
        super().__init__(channel, kernel_size, dilation, dropout)
        self.cnn = nn.Sequential(
            DepthwiseConv1d(channel, channel, kernel_size, stride=1, dilation=dilation, groups=channel),
            nn.BatchNorm1d(channel),
            nn.ReLU(),
            nn.Conv1d(channel, channel, kernel_size=1, stride=1),
            nn.BatchNorm1d(channel),
            nn.ReLU(),
            nn.Dropout(dropout),
        )

    def _convolve(self, y, left_pad):
        y = self.cnn[0](y, left_pad)
        if self.fused_norm:
            y = self.cnn[1](y, relu=True)
            y = self.cnn[4](self.cnn[3](y), relu=True)
            return self.cnn[6](y)
        for layer in list(self.cnn)[1:]:
            y = layer(y)
        return y


class TCN(nn.Module):

    def __init__(self, num_layers: int, channel: int, kernel_size: int, dropout: float = 0.1, block_class=CnnBlock):
        super().__init__()
        self.padding = 0
        self.network = nn.ModuleList()
        for i in range(num_layers):
            dilation = 2**i
            self.padding += (kernel_size - 1) * dilation
            self.network.append(block_class(channel, kernel_size, dilation, dropout))

    def forward(self, x: torch.Tensor, in_cache: torch.Tensor = _empty_cache()) -> Tuple[torch.Tensor, torch.Tensor]:
        """x (B, T, D); in_cache (B, D, C) or empty / None, C the accumulated cache size -> (output (B, T, D), cache (B, D, C))."""
        if in_cache is None:
            in_cache = _empty_cache()
        x = x.transpose(1, 2)  # (B, D, T)
        out_caches = []
        offset = 0
        for block in self.network:
            if in_cache.size(0) > 0:
                c_in = in_cache[:, :, offset:offset + block.padding]
            else:
                c_in = _empty_cache()
            x, c_out = block(x, c_in)
            out_caches.append(c_out)
            offset += block.padding
        x = x.transpose(1, 2)  # (B, T, D)
        new_cache = torch.cat(out_caches, dim=2)
        return x, new_cache
