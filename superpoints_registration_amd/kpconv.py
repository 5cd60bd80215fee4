"""KPConv pyramid preprocessing, encoder and decoder on the HIP library.

Public names follow the reference's ``src/models/backbone_kpconv/kpconv.py`` so
that RegTR-style callers keep working: KPFEncoder (:22-92), KPFDecoder (:95-168), Preprocessor
(:295-418) / PreprocessorGPU (:421-549), batch_grid_subsampling_kpconv (:174),
batch_neighbors_kpconv (:247) and their *_gpu aliases (:217, :265),
calibrate_neighbors (:714, defined in calibration.py).

The pinned contract is the reference's CPU ``Preprocessor`` (its C++
extensions): identical point order at every level, bit-exact barycentres and
neighbour indices.  The reference's ``PreprocessorGPU`` depends on
MinkowskiEngine + PyTorch3D (not vendored, no runnable oracle); here both
names resolve to the same HIP implementation, with the CPU semantics by default.

``neighbor_select='index'`` (argument of Preprocessor / PreprocessorGPU, key of
the config, ``select=ops.SELECT_INDEX`` of batch_neighbors_kpconv) gives the
neighbour rows of the reference's GPU path instead (batch_neighbors_kpconv_gpu,
kpconv.py:265-292 -> pytorch3d.ops.ball_query): per query the K =
neighborhood_limits[level] LOWEST support indices with d2 < r2, ascending,
always K columns, padded with the shadow index.  The two rules keep different
points wherever more than K supports lie in range.  Subsampling keeps the C++
semantics under either rule (MinkowskiEngine's output order is undefined).

Structure differs from the reference: the architecture string list is parsed
ONCE into a pyramid plan (`plan_pyramid`) that both the encoder and the
preprocessor consume, instead of two hand-rolled loops with running state.
"""
from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.nn as nn

from . import decoder, ops, subsample_attrs
from . import tie_order as _tie
from .kpconv_blocks import NearestUpsampleBlock, UnaryBlock, _cu_of, _idx_of, _maxlen_of, block_decider

NEIGHBOR_SELECT = {'nearest': ops.SELECT_NEAREST, 'index': ops.SELECT_INDEX}

_DOWN = ('pool', 'strided')
_STOP = ('global', 'upsample')


@dataclass
class BlockPlan:
    name: str
    level: int       # pyramid level the block reads from
    radius: float    # convolution radius at that level
    in_dim: int
    out_dim: int
    down: bool       # ends the level (strided / pool)


@dataclass
class LevelPlan:
    radius: float    # r_normal of the level (kpconv.py:319, doubles per level :406)
    conv_radius: float   # radius of the conv search (kpconv.py:349-352): the deformable radius when a deformable block
                         # is among the level's non-strided blocks OTHER THAN THE LAST (the reference's layer_blocks[:-1])
    pool_radius: float   # radius of the pool search (kpconv.py:374-377): the deformable radius when the strided block
                         # itself is deformable; the up-sampling search uses twice this one (:385)
    has_conv: bool   # at least one non-strided block -> conv neighbours needed
    down: bool       # the level ends with a strided block -> subsample + pools
    limit: Optional[int]   # neighborhood_limits[level]; None when the config carries none (calibrate_neighbors)


def plan_pyramid(cfg):
    """Parse cfg.architecture into per-block and per-level plans.

    Channel / radius bookkeeping follows KPFEncoder.__init__ (kpconv.py:27-79):
    'simple' halves the advertised width, every strided block doubles radius
    and width and opens a new level.  Level bookkeeping follows
    Preprocessor.forward (kpconv.py:334-408).  A config without neighborhood_limits
    (missing or None: the limits are what calibrate_neighbors is about to find) plans
    the same blocks and levels, with limit=None."""
    limits = getattr(cfg, 'neighborhood_limits', None)
    r = cfg.first_subsampling_dl * cfg.conv_radius
    in_dim, out_dim, level = cfg.in_feats_dim, cfg.first_feats_dim, 0
    blocks: List[BlockPlan] = []
    members: List[List[BlockPlan]] = [[]]
    for name in cfg.architecture:
        if any(s in name for s in _STOP):
            break
        down = any(s in name for s in _DOWN)
        bp = BlockPlan(name, level, r, in_dim, out_dim, down)
        blocks.append(bp)
        members[-1].append(bp)
        in_dim = out_dim // 2 if 'simple' in name else out_dim
        if down:
            level += 1
            r *= 2
            out_dim *= 2
            members.append([])
    if not members[-1]:
        members.pop()
    levels = []
    for l, mem in enumerate(members):
        r = mem[0].radius
        r_deform = r * cfg.deform_radius / cfg.conv_radius if any('deformable' in b.name for b in mem) else r
        convs = [b.name for b in mem if not b.down]
        levels.append(LevelPlan(radius=r,
                                conv_radius=r_deform if any('deformable' in n for n in convs[:-1]) else r,
                                pool_radius=r_deform if mem[-1].down and 'deformable' in mem[-1].name else r,
                                has_conv=any(not b.down for b in mem),
                                down=mem[-1].down,
                                limit=None if limits is None else int(limits[l])))
    return blocks, levels, in_dim


class KPFEncoder(nn.Module):
    """Sequential KPConv encoder.  Attributes `encoder_blocks`,
    `encoder_skips`, `encoder_skip_dims` and the (x, skip_x) return value match
    the reference (kpconv.py:22-92)."""

    def __init__(self, config, d_bottle, increase_channel_when_downsample=True):
        super().__init__()
        if not increase_channel_when_downsample:
            raise NotImplementedError("constant-width pyramids are not used by RegTR")
        blocks, _, final_dim = plan_pyramid(config)
        self._plans = blocks
        self.encoder_blocks = nn.ModuleList(
            block_decider(b.name, b.radius, b.in_dim, b.out_dim, b.level, config) for b in blocks)
        if config.get('deform_fitting_power', 0.0) > 0:
            # the regulariser on the deformed kernel points (the deform_reg subpackage, RegTR.compute_loss) reads each
            # deformable block's last forward: its points and rows stay referenced until the next one
            for m in self.encoder_blocks.modules():
                if hasattr(m, 'keep_reg_inputs'):
                    m.keep_reg_inputs = True
        # skip taps: the input of every strided block, plus the final features
        self.encoder_skips = [i for i, b in enumerate(blocks) if b.down]
        self.encoder_skip_dims = [b.in_dim for b in blocks if b.down]
        arch = list(config.architecture)
        if len(blocks) < len(arch) and 'upsample' in arch[len(blocks)]:
            # a decoder follows (kpconv.py:44-50, :74): the upsample block's own index and input width are listed
            # and the final tap is not added; forward() never reaches that index, so skip_x holds one tensor per
            # strided block
            self.encoder_skips.append(len(blocks))
            self.encoder_skip_dims.append(final_dim)
        else:
            self.encoder_skips.append(len(blocks) - 1)
            self.encoder_skip_dims.append(final_dim)

    def forward(self, x, batch):
        skip_x = []
        for i, block in enumerate(self.encoder_blocks):
            if i in self.encoder_skips:
                skip_x.append(x)
            x = block(x, batch)
        return x, skip_x

    def forward_streamed(self, x, stream):
        """forward() driven by Preprocessor.stream(): every block is launched as soon as its part
        of the pyramid exists.  Same kernels, same operands -> bitwise the result of
        forward(x, meta).  Returns (x, skip_x, meta)."""
        plans = self._plans
        skip_x, i, meta = [], 0, None
        for meta, kind, level in stream:
            while i < len(self.encoder_blocks):
                bp = plans[i]
                ready = bp.level < level or (bp.level == level and (kind == 'down' or not bp.down))
                if not ready:
                    break
                if i in self.encoder_skips:
                    skip_x.append(x)
                x = self.encoder_blocks[i](x, meta)
                i += 1
        assert i == len(self.encoder_blocks), "pyramid ended before the encoder"
        return x, skip_x, meta


class KPFDecoder(nn.Module):
    """Upsampling half of the backbone (kpconv.py:95-168; Predator's dense descriptors -- RegTR itself never builds
    it).  Attributes `decoder_blocks`, `decoder_concats`, the state-dict names and the (x, x_all) return value match
    the reference.  A NearestUpsampleBlock followed by a UnaryBlock runs as ONE projection that gathers while it
    stages its tiles (decoder.upsample_unary): the upsampled and the concatenated tensors are never produced."""

    def __init__(self, config, in_dim, encoder_skip_dims, reduce_channel_when_upsample=True):
        super().__init__()
        out_dim = in_dim
        self.decoder_blocks = nn.ModuleList()
        self.decoder_concats = []
        arch = list(config.architecture)
        # first upsampling block, and the level / radius the encoder ends on
        octave, start_i = 0, 0
        r = config.first_subsampling_dl * config.conv_radius
        for block_i, block in enumerate(arch):
            if 'upsample' in block:
                start_i = block_i
                break
            elif 'pool' in block or 'strided' in block:
                octave += 1
                r *= 2
        for block_i, block in enumerate(arch[start_i:]):
            # a block behind an upsample reads the skip tensor of its level as well
            if block_i > 0 and 'upsample' in arch[start_i + block_i - 1]:
                in_dim += encoder_skip_dims[octave]
                self.decoder_concats.append(block_i)
            self.decoder_blocks.append(block_decider(block, r, in_dim, out_dim, octave, config))
            in_dim = out_dim
            if 'upsample' in block:
                octave -= 1
                r *= 0.5
                if reduce_channel_when_upsample:
                    out_dim = out_dim // 2

    def forward(self, x, skip_x, batch):
        x_all = []
        pyr = len(batch['stack_lengths']) - 1
        blocks = self.decoder_blocks
        i = 0
        while i < len(blocks):
            block = blocks[i]
            nxt = blocks[i + 1] if i + 1 < len(blocks) else None
            if (isinstance(block, NearestUpsampleBlock) and isinstance(nxt, UnaryBlock)
                    and i not in self.decoder_concats):
                # upsample + unary: block i + 1 is in decoder_concats by construction
                pyr -= 1
                y = decoder.upsample_unary(x, skip_x.pop(), _idx_of(batch, 'upsamples', block.layer_ind - 1),
                                           nxt.mlp.weight)
                x = nxt.batch_norm(y, batch['stack_lengths'][pyr], cu=_cu_of(batch, pyr),
                                   slope=1.0 if nxt.no_relu else 0.1, max_len=_maxlen_of(batch, pyr))
                x_all.append(x)
                i += 2
                continue
            if i in self.decoder_concats:
                pyr -= 1
            if isinstance(block, UnaryBlock):
                y = decoder.concat_unary(x, skip_x.pop(), block.mlp.weight)
                x = block.batch_norm(y, batch['stack_lengths'][pyr], cu=_cu_of(batch, pyr),
                                     slope=1.0 if block.no_relu else 0.1, max_len=_maxlen_of(batch, pyr))
            else:
                x = block(x, batch)
            if i in self.decoder_concats:
                x_all.append(x)
            i += 1
        return x, x_all


# --------------------------------------------------------------------------- #
def batch_grid_subsampling_kpconv(points, batches_len, features=None, labels=None, sampleDl=0.1,
                                  max_p=0, verbose=0, random_grid_orient=True,
                                  order=ops.ORDER_REFERENCE):
    """Replaces cpp_subsampling.subsample_batch behind kpconv.py:174-214.
    points [N,3] on the device, batches_len [B] -> (sub_points, sub_lengths).
    With features [N, d] and / or labels [N] or [N, d]: the reference's 3- or 4-tuple (kpconv.py:187-214), (sub_points,
    sub_lengths[, sub_features][, sub_labels]) on the device; sub_labels is int32 [M, ldim] as the reference's wrapper
    returns it (wrapper.cpp:282-284, :309), also for labels of shape [N]."""
    cu = ops.lengths_to_cu(batches_len, points.device)
    if features is not None or labels is not None:
        res = list(subsample_attrs.grid_subsample(points, cu, sampleDl, max_p=max_p, order=order, features=features,
                                                  labels=labels))
        if labels is not None:
            res[-1] = res[-1].reshape(res[0].shape[0], -1).to(torch.int32)
        return tuple(res)
    return ops.grid_subsample(points, cu, sampleDl, max_p=max_p, order=order)


def batch_neighbors_kpconv(queries, supports, q_batches, s_batches, radius, max_neighbors,
                           select=ops.SELECT_NEAREST):
    """Replaces cpp_neighbors.batch_query + the column slice (kpconv.py:247-262).
    Returns int32 [Nq, min(max_count, max_neighbors)], shadow index = Ns.
    select=ops.SELECT_INDEX: the rows of batch_neighbors_kpconv_gpu (kpconv.py:265-292) instead -- the
    max_neighbors lowest support indices in range, ascending, always max_neighbors columns."""
    limit = int(max_neighbors) if max_neighbors > 0 else 128
    idx, _ = ops.radius_neighbors(queries, supports,
                                  ops.lengths_to_cu(q_batches, queries.device),
                                  ops.lengths_to_cu(s_batches, queries.device),
                                  radius, limit, exact_width=True, select=select)
    return idx


batch_grid_subsampling_kpconv_gpu = batch_grid_subsampling_kpconv  # kpconv.py:217
batch_neighbors_kpconv_gpu = batch_neighbors_kpconv                # kpconv.py:265


class _IndexList(list):
    """List of per-level index matrices that holds the kernels' int32 tensors and converts
    an entry to the public dtype (int64, like the reference's torch.long indices) the first
    time it is READ.  The forward pass itself only uses the int32 views, so the three
    [N, limit] int64 copies per level (hundreds of MB per step) are only made for callers
    that actually look at them."""

    def __init__(self, dtype):
        super().__init__()
        self._dtype = dtype

    def _conv(self, i):
        t = list.__getitem__(self, i)
        if t.dtype != self._dtype:
            t = t.to(self._dtype)
            list.__setitem__(self, i, t)
        return t

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._conv(j) for j in range(*i.indices(len(self)))]
        return self._conv(i if i >= 0 else len(self) + i)

    def __iter__(self):
        return (self._conv(i) for i in range(len(self)))


class Preprocessor(nn.Module):
    """Builds the KPConv pyramid metadata for a list of clouds.

    Returns boundary B2 of SURVEY.md section 8b: {'points', 'neighbors',
    'pools', 'upsamples', 'stack_lengths'}, lists over levels; index tensors
    are int64 (`index_dtype`) with shadow index = number of support points;
    the last level's pools / upsamples are (0, 1) placeholders like the
    reference (kpconv.py:389-392).  Private '_' keys carry what the kernels
    want: int32 index views, cu_seqlens, host-side lengths.

    compute_upsamples=False skips the up-sampling search the encoder-only
    RegTR never reads (kpconv.py:384 computes it regardless).
    order=ops.ORDER_CANONICAL emits subsampled points in ascending voxel-key
    order instead of the reference's hash-map order (better gather locality;
    poses agree to rounding, indices are a relabelling).
    neighbor_select: 'nearest' (default: the reference's CPU Preprocessor -- the
    limit nearest supports, by distance, sliced to the widest row) or 'index'
    (the reference's PreprocessorGPU, which RegTR.__init__ of the reference
    hard-wires, qk_regtr_full.py:40: the limit lowest support indices in range,
    ascending, always limit columns); None reads cfg.neighbor_select.  It
    applies to the conv, pool and up-sampling searches; points and lengths do
    not depend on it.
    tie_order: 'index' (default: an equal-distance run of a 'nearest' row is in
    ascending index order) or 'reference' (the order the reference's kd-tree
    search and std::sort leave it in: every matrix equals the reference's CPU
    Preprocessor's, index for index; tie_order.py); None reads cfg.tie_order.
    One kd-tree replay per level serves its conv, pool and up-sampling fix-ups;
    `tie_status` then maps (level, kind) to the latest (rows_fixed, ...) status.
    """

    def __init__(self, cfg, compute_upsamples=True, order=ops.ORDER_REFERENCE,
                 index_dtype=torch.int64, neighbor_select=None, tie_order=None):
        super().__init__()
        self.cfg = cfg
        if neighbor_select is None:
            neighbor_select = cfg.get('neighbor_select', 'nearest')
        if neighbor_select not in NEIGHBOR_SELECT:
            raise ValueError(f"neighbor_select must be 'nearest' or 'index', got {neighbor_select!r}")
        self.neighbor_select = neighbor_select
        if tie_order is None:
            tie_order = cfg.get('tie_order', 'index')
        self.tie_order = _tie.check(tie_order, neighbor_select)
        self.tie_status = {}
        self.compute_upsamples = compute_upsamples
        self.order = order
        self.index_dtype = index_dtype
        # untruncated max row count of every search of the previous forward, keyed (level, kind): a search whose
        # rows were dense last time (more supports in range than 1.5 x the limit: LiDAR-shaped clouds) takes the
        # wave-per-query selection, the others the thread-per-query one (ops.RadiusTable.query; identical rows)
        self._row_counts = {}

    def forward(self, pts: List[torch.Tensor]):
        meta = None
        for meta, _, _ in self.stream(pts):
            pass
        return meta

    def stream(self, pts: List[torch.Tensor]):
        """Generator form of forward(): yields (meta, 'conv' | 'down', level) as soon as what an
        encoder block of that kind needs is in `meta` -- 'conv': points / lengths / conv
        neighbours of the level; 'down': pools (and upsamples) of the level plus the points and
        lengths of the next one.  RegTR runs it on a side stream and launches the encoder blocks
        between the yields (KPFEncoder.forward_streamed): the index work -- small, latency-bound
        kernels and one device->host read per subsampling and per neighbour matrix -- then runs
        beside the convolutions instead of in front of them.  Exhausting the generator leaves
        `meta` exactly as forward() returns it."""
        cfg = self.cfg
        _, levels, _ = plan_pyramid(cfg)
        device = pts[0].device
        points = torch.cat(pts, dim=0).to(torch.float32).contiguous()
        lens_host = [int(p.shape[0]) for p in pts]

        meta = {k: [] for k in ('points', 'stack_lengths')}
        meta.update({k: _IndexList(self.index_dtype) for k in ('neighbors', 'pools', 'upsamples')})
        meta.update(_cu={}, _i32={}, _lens_host=[], _rows_sorted=True, pool_order=[])
        placeholder = torch.zeros((0, 1), dtype=self.index_dtype, device=device)

        def publish(key, level, idx):
            if idx is None:
                meta[key].append(placeholder)
                return
            meta['_i32'][(key, level)] = idx
            meta[key].append(idx)                 # converted to index_dtype on first read
            if key != 'upsamples':                # conv / pool matrices feed KPConvs: tile plan built here, off the main stream
                ops.kpconv_plan_prefetch(idx, plan_ns[0])

        plan_ns = [0]                             # supports of the matrices being published (= points of the current level)

        def open_level(l, points, lens_host, cu):
            meta['points'].append(points)
            meta['stack_lengths'].append(torch.tensor(lens_host, dtype=torch.int32, device=device))
            meta['_cu'][l] = cu
            meta['_lens_host'].append(lens_host)

        # One cell table per (supports, radius): a level's conv and pool searches and the previous level's
        # up-sampling search (radius 2 r = the next level's r) all look into the same one.
        table = [None]
        tree = [None]                             # tie_order='reference': one kd-tree replay per support set

        def search(key, queries, q_cu, supports, s_cu, radius, limit):
            if table[0] is None or not table[0].matches(supports, s_cu, radius):
                table[0] = ops.RadiusTable(supports, s_cu, radius)
            prev = self._row_counts.get(key)
            idx, m = table[0].query(queries, q_cu, limit, dense=None if prev is None else prev > 1.5 * limit,
                                    select=select)
            self._row_counts[key] = m
            if self.tie_order == 'reference':
                if tree[0] is None or not tree[0].matches(supports, s_cu):
                    tree[0] = _tie.ReplayTree(supports, s_cu)
                self.tie_status[key] = tree[0].apply(idx, queries, q_cu, radius, m)
            return idx

        select = NEIGHBOR_SELECT[self.neighbor_select]
        cu = ops.lengths_to_cu(lens_host, device)
        open_level(0, points, lens_host, cu)
        for l, lv in enumerate(levels):
            conv = pool = up = None
            plan_ns[0] = points.shape[0]
            if lv.has_conv:
                conv = search((l, 'conv'), points, cu, points, cu, lv.conv_radius, lv.limit)
            publish('neighbors', l, conv)
            yield meta, 'conv', l
            if lv.down:
                dl = 2 * lv.radius / cfg.conv_radius          # kpconv.py:367
                sub_points, sub_lens = ops.grid_subsample(points, cu, dl, order=self.order)
                sub_lens_host = sub_lens.tolist()
                sub_cu = ops.lengths_to_cu(sub_lens_host, device)
                pool = search((l, 'pool'), sub_points, sub_cu, points, cu, lv.pool_radius, lv.limit)
                # spatial walk order of the level's pooled queries (kpconv_blocks.max_pool): one key + sort pass here,
                # off the main stream, saves the max-pool most of its re-reads of the finer level's features
                meta['pool_order'].append(ops.cell_order(sub_points, sub_cu, dl))
                if self.compute_upsamples:
                    up = search((l, 'up'), points, cu, sub_points, sub_cu, 2 * lv.pool_radius, lv.limit)
            if not lv.down:
                meta['pool_order'].append(None)
            publish('pools', l, pool)
            publish('upsamples', l, up)
            if lv.down:
                points, lens_host, cu = sub_points, sub_lens_host, sub_cu
                open_level(l + 1, points, lens_host, cu)
            yield meta, 'down', l


# kpconv.py:421.  The name keeps the CPU semantics by default, like every caller of it has had so far; the neighbour
# rows the reference's class of this name computes are PreprocessorGPU(cfg, neighbor_select='index').
PreprocessorGPU = Preprocessor

from .calibration import calibrate_neighbors, coverage  # noqa: E402,F401  (kpconv.py:714; needs plan_pyramid above)
