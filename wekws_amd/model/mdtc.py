"""Trainable mirrors of the reference's MDTC backbone (wekws/model/mdtc.py): ``DSDilatedConv1d``, ``TCNBlock``, ``TCNStack``
and ``MDTC`` with the same constructors, state-dict keys and shapes and the same ``forward(x, in_cache) -> (out, cache)``, so
state dicts go both ways (and into the packed inference model, ``wekws_amd.model.kws_model``).

The depthwise convolution of a ``DSDilatedConv1d`` is a ``wekws_amd.model.depthwise.DepthwiseConv1d``: with an empty cache a
``TCNBlock`` calls it with ``left_pad = padding``, so the block's ``F.pad`` copy is not made and, for float32 device tensors,
the HIP kernels run.  With a non-empty cache (streaming) the block does what the reference does:
``torch.cat``, then the convolution.  The pointwise convolutions (``conv1.pointwise`` and ``conv2`` of a ``TCNBlock``) are
constructed as ``nn.Conv1d`` and stay torch's unless ``wekws_amd.model.pointwise.use_device_pointwise_convs`` has swapped them
for ``PointwiseConv1d``s; BatchNorm and ReLU stay torch's unless
``wekws_amd.model.batchnorm.use_device_batchnorms`` has set a block's ``fused_norm``: then each BatchNorm is a
``DeviceBatchNorm1d`` and a ``TCNBlock`` hands ``relu1``, the residual add and ``relu2`` to its calls.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn as nn

from wekws_amd.model.depthwise import DepthwiseConv1d
from wekws_amd.model.tcn import _empty_cache, padded_tail


class DSDilatedConv1d(nn.Module):
    """Dilated depthwise-separable convolution: depthwise ``conv``, ``bn``, ``pointwise``."""

    fused_norm = False      # set by use_device_batchnorms: bn is a DeviceBatchNorm1d (nothing follows it that could be fused)

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, dilation: int = 1, stride: int = 1, bias: bool = True):
        super().__init__()
        self.padding = dilation * (kernel_size - 1)
        self.conv = DepthwiseConv1d(in_channels, in_channels, kernel_size, padding=0, dilation=dilation, stride=stride,
                                    groups=in_channels, bias=bias)
        self.bn = nn.BatchNorm1d(in_channels)
        self.pointwise = nn.Conv1d(in_channels, out_channels, kernel_size=1, padding=0, dilation=1, bias=bias)

    def forward(self, inputs: torch.Tensor, left_pad: int = 0) -> torch.Tensor:
        """``inputs`` with ``left_pad`` zeros in front of every row."""
        return self.pointwise(self.bn(self.conv(inputs, left_pad)))


class TCNBlock(nn.Module):

    fused_norm = False      # set by use_device_batchnorms: bn1 and bn2 are DeviceBatchNorm1ds that apply the ReLUs and the residual add

    def __init__(self, in_channels: int, res_channels: int, kernel_size: int, dilation: int, causal: bool):
        super().__init__()
        self.in_channels = in_channels
        self.res_channels = res_channels
        self.kernel_size = kernel_size
        self.dilation = dilation
        self.causal = causal
        self.padding = dilation * (kernel_size - 1)
        self.half_padding = self.padding // 2
        self.conv1 = DSDilatedConv1d(in_channels=in_channels, out_channels=res_channels, kernel_size=kernel_size, dilation=dilation)
        self.bn1 = nn.BatchNorm1d(res_channels)
        self.relu1 = nn.ReLU()
        self.conv2 = nn.Conv1d(in_channels=res_channels, out_channels=res_channels, kernel_size=1)
        self.bn2 = nn.BatchNorm1d(res_channels)
        self.relu2 = nn.ReLU()

    def forward(self, inputs: torch.Tensor, cache: torch.Tensor = _empty_cache()) -> Tuple[torch.Tensor, torch.Tensor]:
        """inputs (B, D, T); cache (B, D, self.padding) or empty -> (outputs (B, D, T), new cache (B, D, self.padding))."""
        if cache.size(0) == 0:
            new_cache = padded_tail(inputs, self.padding)
            outputs = self.conv1(inputs, self.padding)
        else:
            outputs = torch.cat((cache, inputs), dim=2)
            assert outputs.size(2) > self.padding
            new_cache = outputs[:, :, -self.padding:]
            outputs = self.conv1(outputs, 0)
        if self.fused_norm:
            outputs = self.bn1(outputs, relu=True)
            residual = inputs if self.in_channels == self.res_channels else None
            return self.bn2(self.conv2(outputs), residual=residual, relu=True), new_cache
        outputs = self.relu1(self.bn1(outputs))
        outputs = self.bn2(self.conv2(outputs))
        if self.in_channels == self.res_channels:
            res_out = self.relu2(outputs + inputs)
        else:
            res_out = self.relu2(outputs)
        return res_out, new_cache


class TCNStack(nn.Module):

    def __init__(self, in_channels: int, stack_num: int, stack_size: int, res_channels: int, kernel_size: int, causal: bool):
        super().__init__()
        self.in_channels = in_channels
        self.stack_num = stack_num
        self.stack_size = stack_size
        self.res_channels = res_channels
        self.kernel_size = kernel_size
        self.causal = causal
        self.res_blocks = self.stack_tcn_blocks()
        self.padding = self.calculate_padding()

    def calculate_padding(self) -> int:
        return sum(block.padding for block in self.res_blocks)

    def build_dilations(self):
        return [2**l for _ in range(self.stack_size) for l in range(self.stack_num)]

    def stack_tcn_blocks(self) -> nn.ModuleList:
        dilations = self.build_dilations()
        res_blocks = nn.ModuleList()
        res_blocks.append(TCNBlock(self.in_channels, self.res_channels, self.kernel_size, dilations[0], self.causal))
        for dilation in dilations[1:]:
            res_blocks.append(TCNBlock(self.res_channels, self.res_channels, self.kernel_size, dilation, self.causal))
        return res_blocks

    def forward(self, inputs: torch.Tensor, in_cache: torch.Tensor = _empty_cache()) -> Tuple[torch.Tensor, torch.Tensor]:
        outputs = inputs  # (B, D, T)
        out_caches = []
        offset = 0
        for block in self.res_blocks:
            if in_cache.size(0) > 0:
                c_in = in_cache[:, :, offset:offset + block.padding]
            else:
                c_in = _empty_cache()
            outputs, c_out = block(outputs, c_in)
            out_caches.append(c_out)
            offset += block.padding
        return outputs, torch.cat(out_caches, dim=2)


class MDTC(nn.Module):
    """Multi-scale depthwise temporal convolution: a preprocessing ``TCNBlock``, ``stack_num`` stacks of ``stack_size`` blocks
    with dilations 1, 2, 4, ..., and the sum of the stacks' outputs."""

    def __init__(self, stack_num: int, stack_size: int, in_channels: int, res_channels: int, kernel_size: int, causal: bool):
        super().__init__()
        assert kernel_size % 2 == 1
        self.kernel_size = kernel_size
        assert causal is True, "we now only support causal mdtc"
        self.causal = causal
        self.preprocessor = TCNBlock(in_channels, res_channels, kernel_size, dilation=1, causal=causal)
        self.relu = nn.ReLU()
        self.blocks = nn.ModuleList()
        self.padding = self.preprocessor.padding
        for _ in range(stack_num):
            self.blocks.append(TCNStack(res_channels, stack_size, 1, res_channels, kernel_size, causal))
            self.padding += self.blocks[-1].padding
        self.half_padding = self.padding // 2

    def forward(self, x: torch.Tensor, in_cache: torch.Tensor = _empty_cache()) -> Tuple[torch.Tensor, torch.Tensor]:
        """x (B, T, D); in_cache (B, D, C) or empty / None -> (outputs (B, T, res_channels), cache)."""
        if in_cache is None:
            in_cache = _empty_cache()
        outputs = x.transpose(1, 2)  # (B, D, T)
        outputs_list = []
        out_caches = []
        offset = 0
        if in_cache.size(0) > 0:
            c_in = in_cache[:, :, offset:offset + self.preprocessor.padding]
        else:
            c_in = _empty_cache()
        outputs, c_out = self.preprocessor(outputs, c_in)
        outputs = self.relu(outputs)
        out_caches.append(c_out)
        offset += self.preprocessor.padding
        for block in self.blocks:
            if in_cache.size(0) > 0:
                c_in = in_cache[:, :, offset:offset + block.padding]
            else:
                c_in = _empty_cache()
            outputs, c_out = block(outputs, c_in)
            outputs_list.append(outputs)
            out_caches.append(c_out)
            offset += block.padding
        outputs = torch.zeros_like(outputs_list[-1], dtype=outputs_list[-1].dtype)
        for y in outputs_list:
            outputs = outputs + y
        outputs = outputs.transpose(1, 2)  # (B, T, D)
        return outputs, torch.cat(out_caches, dim=2)
