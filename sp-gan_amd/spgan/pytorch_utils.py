"""metrics/pointnet2/pytorch_utils.py of the reference: SharedMLP, Conv1d, Conv2d, BatchNorm1d, BatchNorm2d and FC with the reference's
constructor signatures and state_dict keys (`layer0.conv.weight`, `layer0.bn.bn.weight`: the BatchNorm wrapper nests), so a reference
state_dict loads with strict=True and the other way round.

The nn.Conv / nn.BatchNorm children are parameter containers.  A SharedMLP of the configuration the set-abstraction and
feature-propagation modules create (1x1 convolutions, bn on every layer or on none, ReLU, no preact, no instance norm) runs a 4-D GPU
tensor on the HIP path: rows [B*H*W, C] -> per layer one GEMM whose epilogue yields the BatchNorm statistics, the previous layer's
BatchNorm + ReLU applied on the operand load (spgan.pointnet2_modules._RowsMLPFn).  Every other configuration (preact=True, another
activation, instance_norm=True, a CPU tensor) runs as the plain torch layers it is made of.
"""
from __future__ import annotations

from typing import List, Tuple

import torch
import torch.nn as nn

Tensor = torch.Tensor


class SharedMLP(nn.Sequential):
    def __init__(self, args: List[int], *, bn: bool = False, activation=nn.ReLU(inplace=True), preact: bool = False, first: bool = False,
                 name: str = "", instance_norm: bool = False):
        super().__init__()
        for i in range(len(args) - 1):
            plain = first and preact and i == 0           # the first layer of a pre-activated first block: no norm, no activation
            self.add_module(name + "layer{}".format(i),
                            Conv2d(args[i], args[i + 1], bn=bn and not plain, activation=None if plain else activation, preact=preact,
                                   instance_norm=instance_norm))
        self.hip_route = (not preact) and (not instance_norm) and isinstance(activation, nn.ReLU) and len(args) > 1
        self.bn = bool(bn)

    def layers(self):
        return list(self.children())

    def forward(self, x: Tensor) -> Tensor:
        if not (self.hip_route and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            return super().forward(x)
        from .pointnet2_modules import rows_mlp
        B, C, H, W = x.shape
        rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
        out = rows_mlp(rows, self, 1, "none", self.training)
        return out.view(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


class _ConvBase(nn.Sequential):
    def __init__(self, in_size, out_size, kernel_size, stride, padding, activation, bn, init, conv=None, batch_norm=None, bias=True,
                 preact=False, name="", instance_norm=False, instance_norm_func=None):
        super().__init__()
        bias = bias and (not bn)
        conv_unit = conv(in_size, out_size, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias)
        init(conv_unit.weight)
        if bias:
            nn.init.constant_(conv_unit.bias, 0)
        normed = in_size if preact else out_size
        bn_unit = batch_norm(normed) if bn else None
        in_unit = instance_norm_func(normed, affine=False, track_running_stats=False) if instance_norm else None

        def around():
            if bn:
                self.add_module(name + "bn", bn_unit)
            if activation is not None:
                self.add_module(name + "activation", activation)
            if not bn and instance_norm:
                self.add_module(name + "in", in_unit)

        if preact:
            around()
        self.add_module(name + "conv", conv_unit)
        if not preact:
            around()


class _BNBase(nn.Sequential):
    def __init__(self, in_size, batch_norm=None, name=""):
        super().__init__()
        self.add_module(name + "bn", batch_norm(in_size))
        nn.init.constant_(self[0].weight, 1.0)
        nn.init.constant_(self[0].bias, 0)


class BatchNorm1d(_BNBase):
    def __init__(self, in_size: int, *, name: str = ""):
        super().__init__(in_size, batch_norm=nn.BatchNorm1d, name=name)


class BatchNorm2d(_BNBase):
    def __init__(self, in_size: int, name: str = ""):
        super().__init__(in_size, batch_norm=nn.BatchNorm2d, name=name)


class Conv1d(_ConvBase):
    def __init__(self, in_size: int, out_size: int, *, kernel_size: int = 1, stride: int = 1, padding: int = 0,
                 activation=nn.ReLU(inplace=True), bn: bool = False, init=nn.init.kaiming_normal_, bias: bool = True, preact: bool = False,
                 name: str = "", instance_norm=False):
        super().__init__(in_size, out_size, kernel_size, stride, padding, activation, bn, init, conv=nn.Conv1d, batch_norm=BatchNorm1d,
                         bias=bias, preact=preact, name=name, instance_norm=instance_norm, instance_norm_func=nn.InstanceNorm1d)


class Conv2d(_ConvBase):
    def __init__(self, in_size: int, out_size: int, *, kernel_size: Tuple[int, int] = (1, 1), stride: Tuple[int, int] = (1, 1),
                 padding: Tuple[int, int] = (0, 0), activation=nn.ReLU(inplace=True), bn: bool = False, init=nn.init.kaiming_normal_,
                 bias: bool = True, preact: bool = False, name: str = "", instance_norm=False):
        super().__init__(in_size, out_size, kernel_size, stride, padding, activation, bn, init, conv=nn.Conv2d, batch_norm=BatchNorm2d,
                         bias=bias, preact=preact, name=name, instance_norm=instance_norm, instance_norm_func=nn.InstanceNorm2d)


class FC(nn.Sequential):
    def __init__(self, in_size: int, out_size: int, *, activation=nn.ReLU(inplace=True), bn: bool = False, init=None, preact: bool = False,
                 name: str = ""):
        super().__init__()
        fc = nn.Linear(in_size, out_size, bias=not bn)
        if init is not None:
            init(fc.weight)
        if not bn:
            nn.init.constant_(fc.bias, 0)

        def around(size):
            if bn:
                self.add_module(name + "bn", BatchNorm1d(size))
            if activation is not None:
                self.add_module(name + "activation", activation)

        if preact:
            around(in_size)
        self.add_module(name + "fc", fc)
        if not preact:
            around(out_size)
