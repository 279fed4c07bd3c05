"""Host-side mirror of the reference's update operator and correlation blocks
(/root/reference/src/modules/droid_net/{corr,gru,droid_net}.py) on top of the HIP kernels.

Module / parameter names match the reference so that `droid.pth` loads with
`load_state_dict` unchanged (src/slam.py:70-81): update.{corr_encoder,flow_encoder,weight,
delta,gru,agg}.* .  `UpdateModule` / `DroidNet` are plain nn.Modules (the definition the checkpoint loads into and
the fp32 reference of the parity tests); the product path is `FusedUpdate`, which evaluates the same operator entirely
on libglorie_hip kernels (csrc/conv.hip, gru.hip, flowenc.hip: implicit-GEMM MFMA convolutions with fused gate
epilogues), and the correlation blocks (`CorrBlock`, `CorrArena`, `OtfCorrBlock`, `AltCorrBlock`) on csrc/corr*.hip.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import droid_backends


def _conv(cin, cout, k):
    return nn.Conv2d(cin, cout, kernel_size=(k, k), padding=(k // 2, k // 2))


def cvx_upsample(data, mask):
    """droid_net.py:9-23: 8x convex upsampling of a per-pixel field, data [N,h,w,dim], mask [N,576,h,w] (logits of the
    9 taps per 8x8 sub-pixel) -> [N,8h,8w,dim].  One glorie_cvx_upsample launch per channel (softmax in fp32, like the
    reference outside autocast); DepthVideo.upsample calls the kernel directly on its buffers."""
    batch, ht, wd, dim = data.shape
    mask = mask.reshape(batch, 576, ht, wd)
    ix = torch.arange(batch, device=data.device)
    out = torch.empty(batch, 8 * ht, 8 * wd, dim, dtype=torch.float32, device=data.device)
    for c in range(dim):
        up = torch.empty(batch, 8 * ht, 8 * wd, dtype=torch.float32, device=data.device)
        droid_backends.cvx_upsample(data[..., c].float().contiguous(), ix, mask.contiguous(), up, softmax_f32=True)
        out[..., c] = up
    return out


def upsample_disp(disp, mask):
    """droid_net.py:26-31"""
    batch, num, ht, wd = disp.shape
    return cvx_upsample(disp.reshape(batch * num, ht, wd, 1), mask.reshape(batch * num, -1, ht, wd)) \
        .view(batch, num, 8 * ht, 8 * wd)


class GradientClip(nn.Module):
    """identity in the forward pass (clipping.py:7-26 only alters gradients)"""

    def forward(self, x):
        return x


class ConvGRU(nn.Module):
    """gru.py:5-33 -- gates see [net, inp] plus a global context vector"""

    def __init__(self, h_planes=128, i_planes=128):
        super().__init__()
        self.do_checkpoint = False
        for name in ("convz", "convr", "convq"):
            setattr(self, name, _conv(h_planes + i_planes, h_planes, 3))
        self.w = _conv(h_planes, h_planes, 1)
        for name in ("convz_glo", "convr_glo", "convq_glo"):
            setattr(self, name, _conv(h_planes, h_planes, 1))

    def forward(self, net, *inputs):
        inp = torch.cat(inputs, dim=1)
        hx = torch.cat([net, inp], dim=1)
        b, c, h, w = net.shape
        glo = (torch.sigmoid(self.w(net)) * net).view(b, c, h * w).mean(-1).view(b, c, 1, 1)
        z = torch.sigmoid(self.convz(hx) + self.convz_glo(glo))
        r = torch.sigmoid(self.convr(hx) + self.convr_glo(glo))
        q = torch.tanh(self.convq(torch.cat([r * net, inp], dim=1)) + self.convq_glo(glo))
        return (1 - z) * net + z * q


def segment_mean(x, ix, num):
    """scatter_mean(x, ix, dim=1) of torch_scatter (droid_net.py:59): x [b,n,...] -> [b,num,...]"""
    out = torch.zeros((x.shape[0], num) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
    out.index_add_(1, ix, x)
    # counts via index_add_ as well: torch.bincount synchronises with the host
    cnt = torch.zeros(num, dtype=torch.float32, device=x.device)
    cnt.index_add_(0, ix, torch.ones(ix.shape[0], dtype=torch.float32, device=x.device))
    cnt = cnt.clamp_(min=1).to(x.dtype)
    return out / cnt.view(1, num, *([1] * (x.dim() - 2)))


class GraphAgg(nn.Module):
    """droid_net.py:34-66"""

    def __init__(self):
        super().__init__()
        self.conv1 = _conv(128, 128, 3)
        self.conv2 = _conv(128, 128, 3)
        self.relu = nn.ReLU(inplace=True)
        self.eta = nn.Sequential(_conv(128, 1, 3), GradientClip(), nn.Softplus())
        self.upmask = nn.Sequential(_conv(128, 8 * 8 * 9, 1))

    def forward(self, net, ii, groups=None):
        """groups = (ix, count) precomputed by the caller avoids the host sync of torch.unique
        (needed for hipGraph capture of the update operator)"""
        batch, num, ch, ht, wd = net.shape
        if groups is None:
            uniq, ix = torch.unique(ii, sorted=True, return_inverse=True)
            groups = uniq.shape[0]
        else:
            ix, groups = groups
        net = self.relu(self.conv1(net.view(batch * num, ch, ht, wd))).view(batch, num, 128, ht, wd)
        net = segment_mean(net, ix, groups).view(-1, 128, ht, wd)
        net = self.relu(self.conv2(net))
        eta = self.eta(net).view(batch, -1, ht, wd)
        upmask = self.upmask(net).view(batch, -1, 8 * 8 * 9, ht, wd)
        return 0.01 * eta, upmask


class UpdateModule(nn.Module):
    """droid_net.py:69-139"""

    def __init__(self):
        super().__init__()
        cor_planes = 4 * (2 * 3 + 1) ** 2
        self.corr_encoder = nn.Sequential(_conv(cor_planes, 128, 1), nn.ReLU(inplace=True),
                                          _conv(128, 128, 3), nn.ReLU(inplace=True))
        self.flow_encoder = nn.Sequential(_conv(4, 128, 7), nn.ReLU(inplace=True),
                                          _conv(128, 64, 3), nn.ReLU(inplace=True))
        self.weight = nn.Sequential(_conv(128, 128, 3), nn.ReLU(inplace=True), _conv(128, 2, 3),
                                    GradientClip(), nn.Sigmoid())
        self.delta = nn.Sequential(_conv(128, 128, 3), nn.ReLU(inplace=True), _conv(128, 2, 3),
                                   GradientClip())
        self.gru = ConvGRU(128, 128 + 128 + 64)
        self.agg = GraphAgg()

    def forward(self, net, inp, corr, flow=None, ii=None, jj=None, groups=None):
        batch, num, ch, ht, wd = net.shape
        if flow is None:
            flow = torch.zeros(batch, num, 4, ht, wd, device=net.device)
        flat = lambda t: t.view(batch * num, -1, ht, wd)
        net = self.gru(flat(net), flat(inp), self.corr_encoder(flat(corr)),
                       self.flow_encoder(flat(flow)))
        delta = self.delta(net).view(batch, num, -1, ht, wd)
        weight = self.weight(net).view(batch, num, -1, ht, wd)
        delta = delta.permute(0, 1, 3, 4, 2)[..., :2].contiguous()
        weight = weight.permute(0, 1, 3, 4, 2)[..., :2].contiguous()
        net = net.view(batch, num, -1, ht, wd)
        if ii is not None:
            eta, upmask = self.agg(net, ii.to(net.device), groups)
            return net, delta, weight, eta, upmask
        return net, delta, weight


class ResidualBlock(nn.Module):
    """extractor.py:4-57 (norm_fn 'instance' | 'none': the two the reference instantiates)"""

    def __init__(self, in_planes, planes, norm_fn='group', stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        mk = {'group': lambda: nn.GroupNorm(num_groups=planes // 8, num_channels=planes),
              'batch': lambda: nn.BatchNorm2d(planes), 'instance': lambda: nn.InstanceNorm2d(planes),
              'none': lambda: nn.Sequential()}[norm_fn]
        self.norm1, self.norm2 = mk(), mk()
        if stride > 1:
            self.norm3 = mk()
        self.downsample = None if stride == 1 else nn.Sequential(
            nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride, padding=0), self.norm3)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class BasicEncoder(nn.Module):
    """extractor.py:63-129: 7x7/2 stem, three pairs of residual blocks (32, 64/2, 128/2), 1x1 head -> 1/8 resolution.
    Runs once per incoming frame (not on the BA-update path): plain torch convolutions."""

    def __init__(self, out_dim, norm_fn='batch'):
        super().__init__()
        DIM = 32
        self.out_dim, self.norm_fn = out_dim, norm_fn
        self.norm1 = {'group': lambda: nn.GroupNorm(num_groups=8, num_channels=DIM), 'batch': lambda: nn.BatchNorm2d(DIM),
                      'instance': lambda: nn.InstanceNorm2d(DIM), 'none': lambda: nn.Sequential()}[norm_fn]()
        self.conv1 = nn.Conv2d(3, DIM, 7, 2, 3)
        self.relu1 = nn.ReLU(inplace=True)
        self.in_planes = DIM
        self.layer1 = self._make_layer(DIM, stride=1)
        self.layer2 = self._make_layer(2 * DIM, stride=2)
        self.layer3 = self._make_layer(4 * DIM, stride=2)
        self.conv2 = nn.Conv2d(4 * DIM, out_dim, kernel_size=(1, 1))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d, nn.GroupNorm)):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _make_layer(self, dim, stride=1):
        layers = [ResidualBlock(self.in_planes, dim, self.norm_fn, stride=stride),
                  ResidualBlock(dim, dim, self.norm_fn, stride=1)]
        self.in_planes = dim
        return nn.Sequential(*layers)

    def forward(self, x):
        b, n, c1, h1, w1 = x.shape
        x = self.relu1(self.norm1(self.conv1(x.view(b * n, c1, h1, w1))))
        x = self.conv2(self.layer3(self.layer2(self.layer1(x))))
        return x.view(b, n, x.shape[1], x.shape[2], x.shape[3])


class DroidNet(nn.Module):
    """droid_net.py:142-147: `.fnet`, `.cnet`, `.update` - what src/slam.py:66-81 constructs and loads droid.pth into"""

    def __init__(self):
        super().__init__()
        self.fnet = BasicEncoder(out_dim=128, norm_fn='instance')
        self.cnet = BasicEncoder(out_dim=256, norm_fn='none')
        self.update = UpdateModule()


class HalfUpdate:
    """Inference copy of an UpdateModule in fp16 + channels_last.

    The reference evaluates the update operator under autocast (factor_graph.py:211), which
    re-casts every fp32 weight to fp16 on every call (39 cast kernels per update) and runs the
    convolutions in NCHW, where MIOpen's implicit-GEMM kernels are wrapped in NCHW<->NHWC
    transposes (16 per update).  This wrapper keeps a half, channels_last copy of the weights
    (rebuilt if a parameter changes) so neither happens: -15 % on the operator at 36 edges."""

    def __init__(self, module):
        self.src = module
        self._ver = None
        self._net = None

    def _sync(self):
        ver = tuple(p._version for p in self.src.parameters())
        if self._ver != ver:
            import copy
            self._net = copy.deepcopy(self.src).eval().half().to(memory_format=torch.channels_last)
            self._ver = ver

    @staticmethod
    def _cl(t):
        b, n, c, h, w = t.shape
        return t.half().view(b * n, c, h, w).contiguous(memory_format=torch.channels_last).view(b, n, c, h, w)

    @torch.no_grad()
    def __call__(self, net, inp, corr, flow=None, ii=None, jj=None, groups=None):
        self._sync()
        return self._net(self._cl(net), self._cl(inp), self._cl(corr), self._cl(flow), ii, jj, groups)


class FusedUpdate:
    """Inference form of an UpdateModule built for gfx950 (scope row A4): fp16 channels-last maps,
    every wide convolution on the implicit-GEMM MFMA kernel of csrc/conv.hip with its consumer
    fused into the epilogue, the rest in the kernels of csrc/gru.hip (update_ops):

      * convz and convr (gru.py:13-14) are one convolution with 256 output channels whose
        epilogue applies the gates (z, r * net); convq's epilogue is the GRU blend; delta[0],
        weight[0] and agg.conv1 (droid_net.py:85-93,38) -- three 3x3 convolutions of the same
        input -- are one with 384 output channels and a bias+ReLU epilogue;
      * torch.cat([net, inp, corr, flow]) never happens: the convolution reads two channel
        segments ([net] or [r*net], and one persistent [N,320,h,w] buffer that the encoders write
        their slices of).  The inp slice is re-filled only when the caller passes a different
        tensor than at the previous call;
      * the 1x1 corr_encoder[0] reads the NCHW output of the correlation lookup as a transposed
        GEMM operand (hipBLASLt) and lands channels-last: no layout pass over the 196-channel map;
      * the global-context vector and its three 1x1 convolutions are two small launches
        (glorie_gru_glo_terms);
      * the 128 -> 2 / 128 -> 1 heads (delta[2], weight[2], agg.eta) are the tap-GEMM + stencil
        kernel glorie_conv3x3_small; GraphAgg's scatter_mean is glorie_segment_mean (fixed order);
        the upmask logits stay channels-last for glorie_cvx_upsample_nhwc.  For a caller that hands over its bookkeeping
        (`book`, fuse_tail) the launches behind the heads' hidden convolution are three: glorie_heads_finish (stencil +
        scatter_mean + target), agg.conv2, glorie_eta_finish (eta head + damping rows + ages).

    No convolution goes through MIOpen (flow_encoder[0] is glorie_flow_conv7).  Same call signature and
    return values as UpdateModule.forward (droid_net.py:106-139); delta, weight and eta come back
    in float32.  Weights are re-packed whenever a parameter of the source module changes."""

    def __init__(self, module, inplace=False):
        """inplace: write the new recurrent state over the `net` argument when that already is an
        fp16 channels-last map (the blend epilogue reads and writes the same element in one lane,
        and no later kernel reads halo rows of the old state) -- callers that replay the update as
        a hipGraph keep one persistent state buffer this way"""
        self.src = module
        self.inplace = inplace
        self.hoist_inp = True       # evaluate the inp part of the gate convolutions once per edge set
        self._pre = None
        # flow encoder / global context on side streams: the branches do overlap (3 hardware queues in the
        # trace) but every kernel involved is throughput-bound and slows down accordingly -- measured
        # 2 % slower per step in an interleaved A/B, so it stays off
        self.parallel = False
        self.glo_stream = True      # the global-context branch on a side stream (see __call__)
        self._streams = None
        self._ver = None
        self._hx = None
        self._inp_key = None      # (tensor kept alive, version) whose values sit in the inp slice of hx
        self._pre_kf, self._pre_map, self._ctx_key = None, None, None   # context term shared per keyframe
        self._flow_pad = None     # zero-padded fp16 motion map (update_ops.PaddedFlow) for callers that pass fp32 flow
        self.fuse_glo = True      # global-context reduction inside the epilogue of its 1x1 convolution
        self.fuse_heads = True    # tap GEMMs of the delta / weight heads inside the epilogue of their hidden convolution
        # flow encoder as one launch (glorie_flow_encoder); GLORIE_FLOW_FUSED=0 keeps its two launches
        self.fuse_flow = os.environ.get("GLORIE_FLOW_FUSED", "1") != "0"
        # stencil + scatter_mean (+ target) as one launch, eta head + bookkeeping as one (glorie_heads_finish, glorie_eta_finish)
        # for callers that pass `book`; GLORIE_TAIL_FUSED=0 keeps the six launches
        self.fuse_tail = os.environ.get("GLORIE_TAIL_FUSED", "1") != "0"
        self.gate_events = None   # a list: (start, end) events of every z|r gate launch are appended (eager steps only)
        self.q_events = None      # the same for the q gate launch and for the heads' hidden convolution (bench.py)
        self.heads_events = None
        self.corr_events = None   # the same for the correlation lookup (+ corr_encoder[0]) launch

    # -- weight packing ----------------------------------------------------------------
    def _sync(self):
        from . import update_ops as U
        ver = tuple(p._version for p in self.src.parameters())
        if self._ver == ver:
            return
        m = self.src
        f32 = lambda b: b.detach().float().contiguous()
        g = m.gru
        W = {}
        W["ce1_t"] = m.corr_encoder[0].weight.detach().view(128, -1).t().half().contiguous()
        W["ce1_b"] = f32(m.corr_encoder[0].bias)
        W["ce1_p"] = OtfCorrBlock.pack_encoder(m.corr_encoder[0].weight)
        W["ce1_cl"] = U.pack_corr_encoder(m.corr_encoder[0].weight)
        W["ce1_dm"] = U.pack_corr_encoder_dm(m.corr_encoder[0].weight)
        W["ce2"], W["ce2_b"] = U.pack_conv_igemm(m.corr_encoder[2].weight, pair=True), f32(m.corr_encoder[2].bias)
        W["fe1"], W["fe1_b"] = U.pack_flow_conv7(m.flow_encoder[0].weight), f32(m.flow_encoder[0].bias)
        W["fe2"], W["fe2_b"] = U.pack_conv_igemm(m.flow_encoder[2].weight, pair=True), f32(m.flow_encoder[2].bias)
        W["zr"] = U.pack_conv_igemm(torch.cat([g.convz.weight, g.convr.weight], 0), pair=True)
        W["q"] = U.pack_conv_igemm(g.convq.weight, pair=True)
        # the same gates split by input channels [net | inp | corr | flow] (gru.py:20-24): the part over the
        # context features inp is evaluated once per edge (`pre`), the rest every iteration
        dyn = lambda wt: torch.cat([wt[:, 0:128], wt[:, 256:448]], 1)
        W["zr_dyn"] = U.pack_conv_igemm(torch.cat([dyn(g.convz.weight), dyn(g.convr.weight)], 0), pair=True)
        W["q_dyn"] = U.pack_conv_igemm(dyn(g.convq.weight), pair=True)
        W["pre"] = U.pack_conv_igemm(torch.cat([g.convz.weight[:, 128:256], g.convr.weight[:, 128:256],
                                                g.convq.weight[:, 128:256]], 0), pair=True)
        W["w"], W["w_b"] = U.pack_conv_igemm(g.w.weight), f32(g.w.bias)
        # glo terms: g[n] = glo[n] @ G + (bias of the 1x1 glo conv + bias of the 3x3 gate conv)
        W["G"] = f32(torch.cat([g.convz_glo.weight.view(128, 128), g.convr_glo.weight.view(128, 128),
                                g.convq_glo.weight.view(128, 128)], 0).t())
        W["G_b"] = f32(torch.cat([g.convz_glo.bias + g.convz.bias, g.convr_glo.bias + g.convr.bias,
                                  g.convq_glo.bias + g.convq.bias]))
        W["h1"] = U.pack_conv_igemm(torch.cat([m.delta[0].weight, m.weight[0].weight, m.agg.conv1.weight], 0))
        W["h1_b"] = f32(torch.cat([m.delta[0].bias, m.weight[0].bias, m.agg.conv1.bias]))
        W["h2"] = U.pack_conv3x3_small([m.delta[2].weight, m.weight[2].weight])
        W["h2_taps"] = U.pack_head_taps([m.delta[2].weight, m.weight[2].weight])
        W["h2_b"] = f32(torch.cat([m.delta[2].bias, m.weight[2].bias]))
        W["a2"], W["a2_b"] = U.pack_conv_igemm(m.agg.conv2.weight, pair=True), f32(m.agg.conv2.bias)
        W["eta"], W["eta_b"] = U.pack_conv3x3_small([m.agg.eta[0].weight]), f32(m.agg.eta[0].bias)
        W["up"], W["up_b"] = U.pack_conv_igemm(m.agg.upmask[0].weight), f32(m.agg.upmask[0].bias)
        W["up_cvx"], W["up_cvx_b"] = U.pack_upmask_conv(m.agg.upmask[0].weight, m.agg.upmask[0].bias)
        self.W = W
        self._ver = ver
        self._inp_key = None        # the hoisted context term was computed with the old weights

    @torch.no_grad()
    def precompute_context(self):
        """conv_z|r|q over the context features of every edge (hx[:, 0:128]) -> self._pre [N,384,h,w] fp16.
        A convolution is linear in its input channels and `inp` never changes while an edge lives, so this
        part of the three gate convolutions (128 of 448 input channels) is evaluated when the edges change
        instead of in every iteration; the gate kernels add it in their epilogue."""
        from . import update_ops as U
        hx = self._hx
        n, _, ht, wd = hx.shape
        if self._pre is None or self._pre.shape[0] != n or self._pre.shape[2:] != hx.shape[2:] \
                or self._pre.device != hx.device:
            self._pre = torch.empty((n, 384, ht, wd), dtype=torch.float16, device=hx.device,
                                    memory_format=torch.channels_last)
        U.conv_igemm(hx[:, 0:128], None, self.W["pre"], 9, 384, self._pre)
        return self._pre

    @staticmethod
    def _cl(t):
        b, n, c, h, w = t.shape
        return t.reshape(b * n, c, h, w).half().contiguous(memory_format=torch.channels_last)

    @staticmethod
    def _agg_groups(ii, groups, dev):
        """(ix int64 [N] contiguous, number of groups) of GraphAgg: the caller's, or unique(ii)"""
        if groups is None:
            uniq, ix = torch.unique(ii.to(dev), sorted=True, return_inverse=True)
            return ix.contiguous(), uniq.shape[0]
        ix, ngroups = groups
        return ix.contiguous(), ngroups

    def _side_streams(self, dev):
        if self._streams is None or self._streams[0].device != dev:
            self._streams = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
        return self._streams

    @torch.no_grad()
    def precompute_shared_context(self, context):
        """context = (table [F,128,h,w] of per-keyframe context features, frames LongTensor [G] (sorted, distinct),
        index [N] -> position in `frames`): the edges of one source keyframe share `inp = table[ii]`
        (factor_graph.py:125-130), so conv_z|r|q over it is evaluated per KEYFRAME (G maps, not N) and the gate
        kernels read it through `pre_map` - 36 edges over 8 keyframes read 29 MB instead of 133 MB per iteration."""
        from . import update_ops as U
        table, frames, index = context
        g = int(frames.shape[0])
        ht, wd = table.shape[-2:]
        x = table[frames].half().contiguous(memory_format=torch.channels_last)
        if self._pre_kf is None or self._pre_kf.shape[0] < g or tuple(self._pre_kf.shape[2:]) != (ht, wd) \
                or self._pre_kf.device != x.device:
            self._pre_kf = torch.empty((max(g, 8), 384, ht, wd), dtype=torch.float16, device=x.device,
                                       memory_format=torch.channels_last)
        U.conv_igemm(x, None, self.W["pre"], 9, 384, self._pre_kf[:g])
        n = int(index.shape[0])
        if self._pre_map is None or self._pre_map.shape[0] < n or self._pre_map.device != x.device:
            self._pre_map = torch.zeros(max(n, 64), dtype=torch.int32, device=x.device)
        self._pre_map[:n].copy_(index)
        return self._pre_kf[:g], self._pre_map[:n]

    def _shared_context(self, context):
        table, frames, index = context
        key = (table.data_ptr(), table._version, frames.data_ptr(), frames._version, index.data_ptr(), index._version,
               int(frames.shape[0]), int(index.shape[0]), self._ver)
        if self._ctx_key != key:
            self.precompute_shared_context(context)
            self._ctx_key = key
            # the key holds addresses: keep the tensors alive, or a later edge set's unique(ii) / inverse tensors can land on
            # the freed blocks with the same shape and version 0 and inherit a stale term
            self._ctx_refs = (table, frames, index)
        return self._pre_kf[:int(frames.shape[0])], self._pre_map[:int(index.shape[0])]

    @torch.no_grad()
    def __call__(self, net, inp, corr, flow=None, ii=None, jj=None, groups=None, context=None, lazy_up=False,
                 weight_out=None, book=None):
        """corr: the looked-up correlation features [1,N,196,h,w], or a callable returning them (it is
        invoked on the caller's stream after the independent branches were forked).
        context (not in the reference): see precompute_shared_context; `inp` is then not read.
        lazy_up: return the upmask logits unevaluated (update_ops.LazyUpmask) for DepthVideo.upsample.
        weight_out: float32 buffer of the confidence weights' size: they are written there (and returned as a view of it).
        book: update_ops.TailBook - the caller's bookkeeping on delta and eta.  With fuse_tail, fuse_heads and ii it is done
        by the operator's own launches (heads conv -> heads_finish -> agg.conv2 -> eta_finish), which sets book.done; else
        it is left to the caller."""
        from . import update_ops as U
        self._sync()
        W = self.W
        batch, num, _, ht, wd = net.shape
        n, hw = batch * num, ht * wd
        dev = net.device
        cl_map = lambda c: torch.empty((n, c, ht, wd), dtype=torch.float16, device=dev,
                                       memory_format=torch.channels_last)
        if self._hx is None or tuple(self._hx.shape) != (n, 320, ht, wd) or self._hx.device != dev:
            self._hx = cl_map(320)                     # [inp | corr features | flow features]
            self._inp_key = None
        hx = self._hx
        net0 = self._cl(net)
        # Three independent producers feed the GRU: the corr encoder (main stream, after the lookup), the
        # flow encoder and the global-context terms.  With self.parallel the latter two run on side
        # streams (parallel branches under hipGraph capture); see __init__ for why that is off.
        main = torch.cuda.current_stream(dev)
        # Round 4: the global-context branch alone (a 1x1 convolution with a per-tile reduction + the small gate-term kernel,
        # 37 us of latency-bound work that needs few CUs) runs on its own stream beside the flow encoder's convolutions:
        # +4.2 % on the step, interleaved A/B (forked behind the flow encoder, beside the lookup, it gains nothing).
        side = self._side_streams(dev) if self.parallel else ((main, self._side_streams(dev)[1]) if self.glo_stream
                                                              else (main, main))
        for st in side:
            if st is not main:
                st.wait_stream(main)
        with torch.cuda.stream(side[0]):
            # flow_encoder (droid_net.py:79-83)
            if isinstance(flow, U.PaddedFlow):
                pf = flow                                  # FactorGraph._motion wrote the padded fp16 map directly
            else:
                if flow is None:
                    flow = torch.zeros(batch, num, 4, ht, wd, device=dev)
                fl = flow.reshape(n, 4, ht, wd).permute(0, 2, 3, 1).float().contiguous()   # no copy for a [.., h, w, 4] motion map
                if self._flow_pad is None or not self._flow_pad.fits(n, ht, wd, dev):
                    self._flow_pad = U.PaddedFlow(n, ht, wd, dev)
                pf = U.flow_pad(fl, self._flow_pad)
            # one launch with the hidden map in LDS (bit-identical); the two launches for an output it does not handle
            if not (self.fuse_flow and U.flow_encoder(pf, W["fe1"], W["fe1_b"], W["fe2"], W["fe2_b"], hx[:, 256:320],
                                                      strict=False)):
                f1 = U.flow_conv7_padded(pf, W["fe1"], W["fe1_b"], cl_map(128))
                U.conv_igemm(f1, None, W["fe2"], 9, 64, hx[:, 256:320], terms=W["fe2_b"], act=U.ACT_RELU)
        shared = context is not None and self.hoist_inp
        with torch.cuda.stream(side[1]):
            if shared:
                pre_kf, pre_map = self._shared_context(context)
            elif self._inp_key is None or self._inp_key[0] is not inp or self._inp_key[1] != inp._version:
                U.bias_act(self._cl(inp), None, U.ACT_NONE, out=hx[:, 0:128])
                self._inp_key = (inp, inp._version)
                if self.hoist_inp:
                    self.precompute_context()
            # global context of the ConvGRU (gru.py:25-31)
            if self.fuse_glo:
                g = U.gru_glo_terms_fused(net0, W["w"], W["w_b"], W["G"], W["G_b"])
            else:
                wn = U.conv_igemm(net0, None, W["w"], 1, 128, cl_map(128))
                g = U.gru_glo_terms(wn, W["w_b"], net0, W["G"], W["G_b"])
        joined = None
        if self.glo_stream and not self.parallel:
            # joined in front of the lookup: the branch is through by then (it started beside the 68 us flow encoder), and the
            # lookup keeps the chip to itself - with the join behind corr_encoder[2] its tail still overlapped the lookup:
            # step +0.4 %, lookup 48 -> 57 us
            main.wait_stream(side[1])
            joined = side[1]
        # corr_encoder (droid_net.py:73-77): 1x1 as a transposed GEMM on the NCHW lookup output
        if hasattr(corr, "encode_into"):
            # volume-free lookup with corr_encoder[0] fused behind it (csrc/corr_otf.hip): the 196-channel map
            # never exists in HBM
            c1 = cl_map(128)
            evc = self.corr_events
            if evc is not None:
                c0e, c1e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                c0e.record()
            corr.encode_into(W, c1)
            if evc is not None:
                c1e.record()
                evc.append((c0e, c1e))
        else:
            if callable(corr):
                corr = corr()                          # the lookup itself, issued behind the forks
            if corr.dim() == 4 and corr.shape[1] == 256 and corr.dtype == torch.float16:
                # channels-last lookup (corr_lookup_tiled_cl): the 1x1 encoder is an implicit-GEMM launch with the
                # bias and the ReLU in its epilogue - no library GEMM over the planar map, no separate bias pass
                c1 = U.conv_igemm(corr, None, W["ce1_cl"], 1, 128, cl_map(128), terms=W["ce1_b"], act=U.ACT_RELU)
            else:
                c1 = torch.matmul(corr.reshape(n, -1, hw).half().transpose(1, 2), W["ce1_t"])
                c1 = c1.view(n, ht, wd, 128).permute(0, 3, 1, 2)
                U.bias_act(c1, W["ce1_b"], U.ACT_RELU)
        U.conv_igemm(c1, None, W["ce2"], 9, 128, hx[:, 128:256], terms=W["ce2_b"], act=U.ACT_RELU)
        for st in side:
            # a second join of the branch joined above (nothing was issued on it since) is not free: in the replayed step it
            # left the chip idle for 6 us between this convolution and the z|r gates (profiles/tail_fused_step_trace.txt)
            if st is not main and st is not joined:
                main.wait_stream(st)
        # ConvGRU (gru.py:20-34)
        z, rnet = cl_map(128), cl_map(128)
        aliased = net0.data_ptr() == net.data_ptr() and net.dtype == torch.float16
        new = net0 if (self.inplace and aliased) else cl_map(128)
        if self.hoist_inp:
            dynx = hx[:, 128:320]
            pre, pmap = (pre_kf, pre_map) if shared else (self._pre, None)
            ev = self.gate_events                         # bench.py: HIP events around the z|r launch inside real steps
            if ev is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            U.conv_igemm(net0, dynx, W["zr_dyn"], 9, 256, z, epilogue=U.EPI_GRU_ZR, terms=g[:, 0:256], net=net0,
                         out2=rnet, pre=pre[:, 0:256], pre_map=pmap)
            if ev is not None:
                e1.record()
                ev.append((e0, e1))
            evq = self.q_events
            if evq is not None:
                q0, q1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                q0.record()
            U.conv_igemm(rnet, dynx, W["q_dyn"], 9, 128, new, epilogue=U.EPI_GRU_Q, terms=g[:, 256:384], net=net0,
                         z=z, pre=pre[:, 256:384], pre_map=pmap)
            if evq is not None:
                q1.record()
                evq.append((q0, q1))
        else:
            U.conv_igemm(net0, hx, W["zr"], 9, 256, z, epilogue=U.EPI_GRU_ZR, terms=g[:, 0:256], net=net0, out2=rnet)
            U.conv_igemm(rnet, hx, W["q"], 9, 128, new, epilogue=U.EPI_GRU_Q, terms=g[:, 256:384], net=net0, z=z)
        net_out = new.view(batch, num, 128, ht, wd)
        tail = book is not None and self.fuse_tail and self.fuse_heads and ii is not None
        # heads (droid_net.py:85-93) + first conv of GraphAgg (droid_net.py:38,53)
        if self.fuse_heads:
            # the heads' hidden maps are consumed in the epilogue of their convolution (tap rows), only the GraphAgg third is stored
            agg_in = cl_map(128)
            evh = self.heads_events
            if evh is not None:
                h0, h1e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                h0.record()
            rows = U.conv_igemm_heads(new, W["h1"], 9, 384, W["h1_b"], W["h2_taps"], 2, out=agg_in)
            if evh is not None:
                h1e.record()
                evh.append((h0, h1e))
            wo = weight_out if (weight_out is not None and weight_out.is_cuda and weight_out.dtype == torch.float32
                                and weight_out.is_contiguous() and weight_out.numel() == n * ht * wd * 2) else None
            if tail:
                ix, ngroups = self._agg_groups(ii, groups, dev)
                dw, agg = U.heads_finish(rows, W["h2_b"], n, ht, wd, 2, 2, (U.ACT_NONE, U.ACT_SIGMOID), agg_in, ix, ngroups,
                                         out_last=wo, coords1=book.coords1, target=book.target)
            else:
                dw = U.conv_stencil(rows, W["h2_b"], n, ht, wd, 2, 2, (U.ACT_NONE, U.ACT_SIGMOID), out_last=wo)
        else:
            h1 = U.conv_igemm(new, None, W["h1"], 9, 384, cl_map(384), terms=W["h1_b"], act=U.ACT_RELU)
            dw = U.conv3x3_small(h1, W["h2"], W["h2_b"], 2, (U.ACT_NONE, U.ACT_SIGMOID))
            agg_in = h1[:, 256:384]
        delta = dw[0].view(batch, num, ht, wd, 2)
        weight = dw[1].view(batch, num, ht, wd, 2) if (not self.fuse_heads or wo is None) else \
            weight_out.view(batch, num, ht, wd, 2)
        if ii is None:
            return net_out, delta, weight
        # GraphAgg (droid_net.py:50-66): mean over edges with the same source keyframe
        if not tail:
            ix, ngroups = self._agg_groups(ii, groups, dev)
            agg = U.segment_mean(agg_in, ix, ngroups)
        a2 = torch.empty((ngroups, 128, ht, wd), dtype=torch.float16, device=dev,
                         memory_format=torch.channels_last)
        U.conv_igemm(agg, None, W["a2"], 9, 128, a2, terms=W["a2_b"], act=U.ACT_RELU)
        eta = None
        if tail:
            eta = U.eta_finish(a2, W["eta"], W["eta_b"], book.frames, book.damping_table, book.damping_ba, book.ep, book.age,
                               scale=0.01, strict=False)
        if eta is None:
            eta = U.conv3x3_small(a2, W["eta"], W["eta_b"], 1, (U.ACT_SOFTPLUS,), scale=0.01)
            if tail:
                # a map too wide for eta_finish's row blocks: the eta half of the bookkeeping as its own launch (the target
                # is written already)
                L = U.L
                L.check(L.load().glorie_update_bookkeeping(
                    None, None, None, 0, L.ptr(eta), L.ptr(book.frames), L.ptr(book.damping_table), L.ptr(book.damping_ba),
                    ngroups, hw, book.ep, L.ptr(book.age), int(book.age.numel()) if book.age is not None else 0,
                    L.stream_ptr()), "glorie_update_bookkeeping")
        if tail:
            book.done = True
        if lazy_up:
            # the caller only hands the logits to DepthVideo.upsample: convolution + convex upsampling run there as one
            # launch (glorie_conv_upsample), the 576-channel map is never stored
            return net_out, delta, weight, eta.view(batch, ngroups, ht, wd), U.LazyUpmask(a2, W["up_cvx"], W["up_cvx_b"])
        up = torch.empty((ngroups, 576, ht, wd), dtype=torch.float16, device=dev,
                         memory_format=torch.channels_last)
        U.conv_igemm(a2, None, W["up"], 1, 576, up, terms=W["up_b"])
        return net_out, delta, weight, eta.view(batch, ngroups, ht, wd), up.view(batch, ngroups, 576, ht, wd)


# --------------------------------------------------------------------------------------
# correlation blocks
# --------------------------------------------------------------------------------------
class CorrSampler(torch.autograd.Function):
    """corr_index_forward with its adjoint (corr.py:7-22): gradient for the volume, none for the coordinates"""

    @staticmethod
    def forward(ctx, volume, coords, radius):
        ctx.save_for_backward(volume, coords)
        ctx.radius = radius
        corr, = droid_backends.corr_index_forward(volume, coords, radius)
        return corr

    @staticmethod
    def backward(ctx, grad_output):
        volume, coords = ctx.saved_tensors
        grad_output = grad_output.contiguous()
        grad_volume, = droid_backends.corr_index_backward(volume, coords, grad_output, ctx.radius)
        return grad_volume, None, None


class CorrLayer(torch.autograd.Function):
    """altcorr_forward with its adjoint (corr.py:79-94): gradients for both feature maps, zeros for the coordinates"""

    @staticmethod
    def forward(ctx, fmap1, fmap2, coords, r):
        ctx.r = r
        ctx.save_for_backward(fmap1, fmap2, coords)
        corr, = droid_backends.altcorr_forward(fmap1, fmap2, coords, ctx.r)
        return corr

    @staticmethod
    def backward(ctx, grad_corr):
        fmap1, fmap2, coords = ctx.saved_tensors
        grad_corr = grad_corr.contiguous()
        fmap1_grad, fmap2_grad, coords_grad = droid_backends.altcorr_backward(fmap1, fmap2, coords, grad_corr, ctx.r)
        return fmap1_grad, fmap2_grad, coords_grad, None


class _PyramidLookup(torch.autograd.Function):
    """The fused lookup of CorrBlock.__call__ under autograd: forward IS the corr_lookup_pyramid call of the no-grad path
    (bit-identical values), backward the one-launch adjoint of all levels.  apply(coords, radius, *levels)."""

    @staticmethod
    def forward(ctx, coords, radius, *pyramid):
        ctx.save_for_backward(coords)
        ctx.radius = radius
        ctx.shapes = [tuple(v.shape) for v in pyramid]
        return droid_backends.corr_lookup_pyramid(list(pyramid), coords, radius)

    @staticmethod
    def backward(ctx, grad):
        coords, = ctx.saved_tensors
        grads = droid_backends.corr_lookup_pyramid_backward(ctx.shapes, coords, grad.contiguous(), ctx.radius)
        return (None, None) + tuple(grads)


class CorrBlock:
    """All-pairs correlation pyramid + windowed lookup (corr.py:25-76).

    The pyramid is built with torch (fp16 GEMM under autocast, like the reference) and kept
    per edge; the lookup of all 4 levels + the channel concatenation is one HIP launch.

    tiled (default on CUDA for radius 3): every plane is re-stored once, at construction, as 64-byte
    blocks of 4 rows x 8 columns (droid_backends.tile_corr_level) and looked up by the tiled kernel:
    same values bit for bit, 35 % less HBM traffic per lookup.  `corr_pyramid` then holds
    [N*h1*w1, plane_l] tensors instead of the reference's [N, h1, w1, h2>>l, w2>>l].

    Gradients: with gradients enabled and feature maps that require them the block is differentiable w.r.t. both maps
    (matmul and avg_pool2d through torch, the lookup through _PyramidLookup).  The tiled re-store is a custom kernel that
    cuts the graph, so tiled=None then resolves to the row-major pyramid and an explicit tiled=True raises."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=3, tiled=None):
        self.num_levels = num_levels
        self.radius = radius
        corr = CorrBlock.corr(fmap1, fmap2)
        batch, num, h1, w1, h2, w2 = corr.shape
        self.dims = (h1, w1, h2, w2)
        needs_grad = torch.is_grad_enabled() and corr.requires_grad
        if tiled and needs_grad:
            raise RuntimeError("CorrBlock: tiled=True stores the pyramid with a kernel that has no gradient; use tiled=None "
                               "or tiled=False with feature maps that require grad (or build the block under no_grad)")
        if tiled is None:
            tiled = corr.is_cuda and radius == 3 and (h1 * w1) % 8 == 0 and corr.dtype == torch.float16 and not needs_grad
        self.tiled = bool(tiled)
        corr = corr.reshape(batch * num * h1 * w1, 1, h2, w2)
        self.corr_pyramid = []
        for i in range(num_levels):
            if self.tiled:
                self.corr_pyramid.append(droid_backends.tile_corr_level(corr[:, 0]))
            else:
                self.corr_pyramid.append(corr.view(batch * num, h1, w1, h2 // 2 ** i, w2 // 2 ** i))
            if i + 1 < num_levels:
                corr = F.avg_pool2d(corr, kernel_size=2, stride=2)

    @staticmethod
    def corr(fmap1, fmap2):
        batch, num, dim, ht, wd = fmap1.shape
        a = fmap1.reshape(batch * num, dim, ht * wd) / 4.0
        b = fmap2.reshape(batch * num, dim, ht * wd) / 4.0
        return torch.matmul(a.transpose(1, 2), b).view(batch, num, ht, wd, ht, wd)

    def __call__(self, coords, channels_last=False):
        batch, num, ht, wd, _ = coords.shape
        if channels_last and self.tiled and self.num_levels == 4 and self.radius == 3:
            return droid_backends.corr_lookup_tiled_cl(self.corr_pyramid, coords.reshape(batch * num, ht, wd, 2).float()
                                                       .contiguous(), self.dims[2], self.dims[3], interleaved=True)
        c = coords.permute(0, 1, 4, 2, 3).contiguous().view(batch * num, 2, ht, wd).float()
        if self.tiled:
            out = droid_backends.corr_lookup_pyramid_tiled(self.corr_pyramid, c, self.dims[2], self.dims[3])
        else:
            pyr = [v if v.is_contiguous() else v.contiguous() for v in self.corr_pyramid]
            if torch.is_grad_enabled() and any(v.requires_grad for v in pyr):
                out = _PyramidLookup.apply(c, self.radius, *pyr)     # coordinates get no gradient (corr.py:22)
            else:
                out = droid_backends.corr_lookup_pyramid(pyr, c, self.radius)
        return out.view(batch, num, -1, ht, wd)

    @staticmethod
    def _with_slack(rows):
        """copy a list of [P_i, plane] tensors into one allocation with a spare plane on either side"""
        total = sum(r.shape[0] for r in rows)
        store = torch.zeros((total + 2, rows[0].shape[1]), dtype=rows[0].dtype, device=rows[0].device)
        at = 1
        for r in rows:
            store[at:at + r.shape[0]] = r
            at += r.shape[0]
        return store[1:total + 1]

    def cat(self, other):
        if self.tiled != other.tiled:
            raise RuntimeError("cannot concatenate tiled and row-major correlation pyramids")
        if self.tiled:
            self.corr_pyramid = [self._with_slack([a, b]) for a, b in zip(self.corr_pyramid, other.corr_pyramid)]
        else:
            self.corr_pyramid = [torch.cat([a, b], 0) for a, b in zip(self.corr_pyramid, other.corr_pyramid)]
        return self

    def __getitem__(self, index):
        if self.tiled:
            hw = self.dims[0] * self.dims[1]
            self.corr_pyramid = [self._with_slack([v.view(-1, hw, v.shape[1])[index].reshape(-1, v.shape[1])])
                                 for v in self.corr_pyramid]
        else:
            self.corr_pyramid = [v[index] for v in self.corr_pyramid]
        return self


class CorrArena:
    """The correlation pyramids of a FactorGraph's edges in ONE slot-indexed store (scope row A1).

    The reference keeps a CorrBlock per graph whose `cat` / `__getitem__` copy every volume of every level through
    torch.cat and boolean masks whenever an edge is added or removed (corr.py:55-65, factor_graph.py:126,161:
    61 MB per edge at 60x80).  Here an edge is built ONCE (one launch: all four levels in the lookup's layout) into a
    free slot and stays there; adding / removing edges edits the int32 slot list the lookup kernel indirects through.
    Capacity grows geometrically (the only copy that can ever happen).

    layout "dm" (default for 4 levels): displacement-major, source-tiled lines (csrc/corr_dm.hip) - neighbouring source
    pixels share the 128-byte lines their windows read, and corr_encoder[0] can run inside the lookup launch
    (`lookup_encode`).  layout "tiled": per-pixel planes in 4x8 blocks (csrc/corr.hip, rounds 1-2; what other pyramid shapes
    fall back to, and what the layout-agreement tests pass explicitly).

    Inference only: building a slot and both lookups (`lookup_encode` included) are custom kernels without an adjoint, so
    no gradient reaches the feature maps through an arena.  Use CorrBlock or AltCorrBlock with gradients."""

    def __init__(self, h, w, device, num_levels=4, radius=3, capacity=16, layout=None):
        assert radius == 3
        self.h, self.w, self.num_levels, self.radius = h, w, num_levels, radius
        self.device = torch.device(device)
        if layout is None:
            layout = "dm"
        if num_levels != 4 or (h >> 3) < 1 or (w >> 3) < 1 or w > 112:
            layout = "tiled"                 # the displacement-major lookup is the 4-level, radius-3 form only
        if layout not in ("dm", "tiled"):
            raise ValueError(f"CorrArena: unknown layout {layout!r}")
        self.layout = layout
        if layout == "dm":
            self.planes = [int(np.prod(droid_backends.dm_shape(h, w, l))) * 64 for l in range(num_levels)]
        else:
            self.planes = [(((h >> l) + 3) // 4) * (((w >> l) + 7) // 8) * 32 for l in range(num_levels)]
        self.capacity = 0
        self.levels = None
        self.free = []
        self.slots = torch.zeros(0, dtype=torch.int32, device=self.device)      # slot of edge n, in edge order
        self._host_slots = []
        self._grow(capacity)

    @property
    def tiled(self):
        return True

    def __len__(self):
        return len(self._host_slots)

    def _grow(self, capacity):
        hw = self.h * self.w
        new = []
        for l, pl in enumerate(self.planes):
            if self.layout == "dm":
                t = torch.zeros((capacity, pl), dtype=torch.float16, device=self.device)
                if self.levels is not None:
                    t[:self.capacity] = self.levels[l]
            else:
                # one spare plane on either side: read slack of the unaligned block-row loads of the lookup
                t = torch.zeros((capacity * hw + 2, pl), dtype=torch.float16, device=self.device)
                if self.levels is not None:
                    t[1:self.capacity * hw + 1] = self.levels[l][1:self.capacity * hw + 1]
            new.append(t)
        self.free += list(range(capacity - 1, self.capacity - 1, -1))
        self.levels, self.capacity = new, capacity

    def views(self):
        if self.layout == "dm":
            return list(self.levels)
        hw = self.h * self.w
        return [t[1:self.capacity * hw + 1] for t in self.levels]

    def add(self, fmaps_cl, fi, fj):
        """build the pyramids of new edges (source frames fi, target frames fj: int64 device tensors indexing the
        channels-last, 1/4-scaled maps fmaps_cl [F, h*w, 128]) and append them to the edge list"""
        import ctypes
        from . import _lib as L
        n = int(fi.shape[0])
        if n == 0:
            return
        while len(self.free) < n:
            self._grow(max(self.capacity * 3 // 2, self.capacity + n, 16))
        take = [self.free.pop() for _ in range(n)]
        new_slots = torch.tensor(take, dtype=torch.int32, device=self.device)
        v = self.views()
        arr = (ctypes.c_void_p * self.num_levels)(*[t.data_ptr() for t in v])
        fn = L.load().glorie_corr_dm_build if self.layout == "dm" else L.load().glorie_corr_build
        L.check(fn(L.ptr(fmaps_cl), L.ptr(fi.contiguous()), L.ptr(fj.contiguous()), L.ptr(new_slots),
                   ctypes.cast(arr, ctypes.c_void_p), self.num_levels, n, self.h, self.w,
                   int(fmaps_cl.shape[-1]), L.stream_ptr()), "glorie_corr_build")
        self._host_slots += take
        self.slots = torch.cat([self.slots, new_slots])

    def keep(self, mask_host):
        """drop the edges whose mask entry is False: their slots return to the free list, nothing moves"""
        kept = []
        for s_, k in zip(self._host_slots, mask_host):
            if k:
                kept.append(s_)
            else:
                self.free.append(s_)
        self._host_slots = kept
        self.slots = torch.tensor(kept, dtype=torch.int32, device=self.device)

    def _coords4(self, coords):
        batch, num, ht, wd, _ = coords.shape
        N = batch * num
        if N != len(self._host_slots):
            raise RuntimeError(f"CorrArena holds {len(self._host_slots)} edges, coords has {N}")
        return coords.reshape(N, ht, wd, 2).float().contiguous()

    def __call__(self, coords, channels_last=False):
        """channels_last: the [N,256,h,w] fp16 map (channel l*64 + dy*8 + dx, what FusedUpdate's 1x1 encoder consumes)
        instead of the reference's [batch, num, 196, h, w]"""
        import ctypes
        from . import _lib as L
        batch, num, ht, wd, _ = coords.shape
        N = batch * num
        if self.layout == "dm":
            cl = droid_backends.corr_dm_lookup(self.views(), self._coords4(coords), self.h, self.w, slots=self.slots,
                                               interleaved=True)
            return cl if channels_last else droid_backends.cl_to_planar(cl).view(batch, num, -1, ht, wd)
        if N != len(self._host_slots):
            raise RuntimeError(f"CorrArena holds {len(self._host_slots)} edges, coords has {N}")
        if channels_last and self.num_levels == 4:
            return droid_backends.corr_lookup_tiled_cl(self.views(), coords.reshape(N, ht, wd, 2).float().contiguous(),
                                                       self.h, self.w, slots=self.slots, interleaved=True)
        c = coords.permute(0, 1, 4, 2, 3).contiguous().view(N, 2, ht, wd).float()
        out = torch.empty((N, self.num_levels * 49, ht, wd), dtype=torch.float16, device=c.device)
        v = self.views()
        arr = (ctypes.c_void_p * self.num_levels)(*[t.data_ptr() for t in v])
        L.check(L.load().glorie_corr_lookup_arena(ctypes.cast(arr, ctypes.c_void_p), self.num_levels, L.ptr(self.slots),
                                                  L.ptr(c), L.ptr(out), N, ht, wd, self.h, self.w, L.stream_ptr()),
                "glorie_corr_lookup_arena")
        return out.view(batch, num, -1, ht, wd)

    def lookup_encode(self, coords, enc_w, enc_b, enc_out, want_corr=False):
        """layout "dm" only: lookup + corr_encoder[0] in one launch; relu(W corr + b) goes to `enc_out` (channels-last fp16
        [N,128,h,w] or a 128-channel slice), the 256-channel lookup itself is returned only if asked for"""
        if self.layout != "dm":
            raise RuntimeError("lookup_encode needs the displacement-major layout")
        return droid_backends.corr_dm_lookup(self.views(), self._coords4(coords), self.h, self.w, slots=self.slots,
                                             interleaved=True, want_corr=want_corr, enc_w=enc_w, enc_b=enc_b,
                                             enc_out=enc_out)

    def level(self, l):
        """row-major volumes [N, h, w, h>>l, w>>l] of the current edges (tests / debugging: copies)"""
        hw = self.h * self.w
        hl, wl = self.h >> l, self.w >> l
        if self.layout == "dm":
            return droid_backends.dm_to_rowmajor(self.views()[l][self.slots.long()], self.h, self.w, l)
        nby, nbx = (hl + 3) // 4, (wl + 7) // 8
        v = self.views()[l].view(self.capacity, hw, nby, nbx, 4, 8)[self.slots.long()]
        v = v.permute(0, 1, 2, 4, 3, 5).reshape(len(self), hw, nby * 4, nbx * 8)[:, :, :hl, :wl]
        return v.reshape(len(self), self.h, self.w, hl, wl)


class ArenaLookup:
    """one pending lookup of a displacement-major CorrArena that FusedUpdate runs with corr_encoder[0] fused behind it"""

    def __init__(self, arena, coords):
        self.arena, self.coords = arena, coords

    def encode_into(self, W, out):
        self.arena.lookup_encode(self.coords, W["ce1_dm"], W["ce1_b"], out)

    def __call__(self):
        return self.arena(self.coords, channels_last=True)


class AltCorrBlock:
    """Volume-free correlation for long graphs (corr.py:79-145).  With gradients enabled and feature maps that require them
    the lookup goes through CorrLayer (gradients for the maps of both frames); otherwise it is the plain forward call."""

    def __init__(self, fmaps, num_levels=4, radius=3):
        self.num_levels = num_levels
        self.radius = radius
        B, N, C, H, W = fmaps.shape
        f = fmaps.view(B * N, C, H, W) / 4.0
        self.pyramid = []
        for i in range(num_levels):
            self.pyramid.append(f.permute(0, 2, 3, 1).contiguous().view(B, N, H // 2 ** i, W // 2 ** i, C))
            if i + 1 < num_levels:                 # maps whose last level is 1 x 1 (8 x 12 at 4 levels) have nothing left to pool
                f = F.avg_pool2d(f, kernel_size=2, stride=2)

    def corr_fn(self, coords, ii, jj):
        B, N, H, W, S, _ = coords.shape
        coords = coords.permute(0, 1, 4, 2, 3, 5)
        outs = []
        for i in range(self.num_levels):
            f1 = self.pyramid[0][:, ii]
            f2 = self.pyramid[i][:, jj]
            c = (coords / 2 ** i).reshape(B * N, S, H, W, 2).contiguous()
            f1 = f1.reshape((B * N,) + f1.shape[2:]).float().contiguous()
            f2 = f2.reshape((B * N,) + f2.shape[2:]).float().contiguous()
            if torch.is_grad_enabled() and (f1.requires_grad or f2.requires_grad):
                corr = CorrLayer.apply(f1, f2, c.float(), self.radius)    # a zero gradient for the coordinates (corr.py:94)
            else:
                corr, = droid_backends.altcorr_forward(f1, f2, c.float(), self.radius)
            outs.append(corr.view(B, N, S, -1, H, W).permute(0, 1, 3, 4, 5, 2))
        return torch.cat(outs, dim=2)

    def __call__(self, coords, ii, jj):
        squeeze = coords.dim() == 5
        if squeeze:
            coords = coords.unsqueeze(-2)
        corr = self.corr_fn(coords, ii, jj)
        if squeeze:
            corr = corr.squeeze(-1)
        return corr.contiguous()


class FusedLookup:
    """one pending lookup of an OtfCorrBlock that FusedUpdate runs with corr_encoder[0] fused behind it"""

    def __init__(self, block, coords, ii, jj):
        self.block, self.coords, self.ii, self.jj = block, coords, ii, jj

    def encode_into(self, W, out):
        self.block.lookup_encode(self.coords, self.ii, self.jj, W["ce1_p"], W["ce1_b"], out)

    def __call__(self):
        return self.block(self.coords, self.ii, self.jj)


class OtfCorrBlock:
    """Volume-free correlation on the matrix cores (csrc/corr_otf.hip): same call contract as
    AltCorrBlock (`OtfCorrBlock(fmaps)(coords, ii, jj)` -> [B, N, 196, H, W]) and the values a
    CorrBlock volume lookup returns up to fp16 rounding, without the 61 MB/edge volume.
    fmaps: [1, F, C, H, W] (video.fmaps viewed like factor_graph.py:266-268).

    Inference only: neither the lookup nor `lookup_encode` (the lookup with corr_encoder[0] fused behind it) has an adjoint;
    AltCorrBlock is the volume-free block that differentiates."""

    def __init__(self, fmaps, num_levels=4, radius=3):
        assert radius == 3
        self.num_levels = num_levels
        self.radius = radius
        B, N, C, H, W = fmaps.shape
        f = fmaps.view(B * N, C, H, W).half() / 4.0
        self.shape = (H, W, C)
        self.levels = []
        for i in range(num_levels):
            self.levels.append(f.permute(0, 2, 3, 1).reshape(B * N, -1, C).contiguous())
            if i + 1 < num_levels:
                f = F.avg_pool2d(f, kernel_size=2, stride=2)

    def __call__(self, coords, ii, jj):
        import ctypes
        from . import _lib as L
        batch, num, ht, wd, _ = coords.shape
        c = coords.permute(0, 1, 4, 2, 3).contiguous().view(batch * num, 2, ht, wd).float()
        H, W, C = self.shape
        out = torch.empty(batch * num, self.num_levels * 49, ht, wd, dtype=torch.float16, device=c.device)
        arr = (ctypes.c_void_p * self.num_levels)(*[v.data_ptr() for v in self.levels])
        L.check(L.load().glorie_corr_otf(L.ptr(self.levels[0]), ctypes.cast(arr, ctypes.c_void_p),
                                         self.num_levels, L.ptr(c), L.ptr(ii.contiguous()), L.ptr(jj.contiguous()),
                                         L.ptr(out), batch * num, H, W, C, L.stream_ptr()), "glorie_corr_otf")
        return out.view(batch, num, -1, ht, wd)

    @staticmethod
    def pack_encoder(weight):
        """corr_encoder[0].weight [128,196,1,1] -> fp16 [128,224] in the kernel's staging order
        (k = level*56 + row*8 + tap, tap 7 = zero pad; include/glorie_hip.h: glorie_corr_otf_encode)"""
        w = weight.detach().reshape(128, 4, 7, 7)                      # [o][l][i][j]
        p = torch.zeros(128, 4, 7, 8, dtype=torch.float16, device=weight.device)   # [o][l][j][i]
        p[..., :7] = w.permute(0, 1, 3, 2).half()
        return p.reshape(128, 224).contiguous()

    def lookup_encode(self, coords, ii, jj, enc_w, enc_b, enc_out, want_corr=False):
        """lookup + fused corr_encoder[0]: writes relu(W corr + b) into `enc_out`, a channels-last fp16 map
        [N,128,h,w] (or a 128-channel slice of a wider one); returns the 196-channel map only if asked to"""
        import ctypes
        from . import _lib as L
        from . import update_ops as U
        batch, num, ht, wd, _ = coords.shape
        c = coords.permute(0, 1, 4, 2, 3).contiguous().view(batch * num, 2, ht, wd).float()
        H, W, C = self.shape
        if self.num_levels != 4 or tuple(enc_out.shape) != (batch * num, 128, ht, wd):
            raise RuntimeError("lookup_encode: 4 levels and an [N,128,h,w] output map expected")
        stride = U._rows(enc_out, "enc_out")
        out = torch.empty(batch * num, 196, ht, wd, dtype=torch.float16, device=c.device) if want_corr else None
        arr = (ctypes.c_void_p * 4)(*[v.data_ptr() for v in self.levels])
        L.check(L.load().glorie_corr_otf_encode(L.ptr(self.levels[0]), ctypes.cast(arr, ctypes.c_void_p), 4, L.ptr(c),
                                                L.ptr(ii.contiguous()), L.ptr(jj.contiguous()), L.ptr(out),
                                                batch * num, H, W, C, L.ptr(enc_w), L.ptr(enc_b), L.ptr(enc_out),
                                                stride, L.stream_ptr()), "glorie_corr_otf_encode")
        return out.view(batch, num, -1, ht, wd) if want_corr else None
