"""RegTR on the HIP library -- drop-in for the forward pass of the reference's
``src/models/qk_regtr_full.py`` (RegTR.forward :126-311, softmax_correlation
:423-672): same constructor argument (a flat config), same batch dict in
(`src_xyz`, `tgt_xyz` lists), same output dict keys, same state-dict names
 so reference checkpoints load.

Differences by design (documented in DESIGN.md):
  * tokens stay packed from the encoder to the pose head; no (L,B,D) padding,
    no per-pair Python loop in the matching head;
  * `attn` (the dense N x M dual-softmax matrices) is not materialised; the
    entry is a list of None unless `return_attn=True`;
  * the cross-encoder's attention maps (transformers.py:61-82) are recorded only with
    `RegTR(cfg, record_attn=True)`: the encoder then runs operator by operator (not the fused
    chains) and `model.transformer_encoder.get_attentions()` returns the reference's stacked
    (num_layers, B, L, S) maps, padded to the longest src / tgt cloud with zeros;
  * the config-off refinements of softmax_correlation (ratio test, median threshold, overlap
    weighting, top-k pruning, LGR, RANSAC -- qk_regtr_full.py:370-421, :465-556) are available
    on the inference path (`_refined_pose`: one library call for all pairs); the two dead "affinity" switches
    (use_attn_affinity raises in the reference itself, use_corr_affinity) stay unsupported;
  * training: with gradients enabled every operator runs through its explicit HIP backward
    (autograd.py), so `compute_loss(model(batch), batch)['total'].backward()` fills the
    same parameter gradients as the reference's training_step (generic_reg_model.py:82-84);
    under torch.no_grad() the forward is the plain inference path;
  * a batch may hold `clouds` and `pairs` (indices into the clouds) instead of `src_xyz` / `tgt_xyz`: every cloud is
    then encoded once for all the pairs that use it, in training as well (shared_clouds.py).
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import _concurrency, ops, shared_clouds
from .kpconv import NEIGHBOR_SELECT, KPFEncoder, Preprocessor
from .transformers import (PositionEmbeddingCoordsSine, PositionEmbeddingLearned, TransformerCrossEncoder,
                           TransformerCrossEncoderLayer, make_segments)


class _BilinearW(nn.Module):
    """Parameter holder for the loss-only `feature_criterion(.un).W` tensors
    (models/losses/feature_loss.py:246-260) so that state dicts round-trip."""

    def __init__(self, d):
        super().__init__()
        self.W = nn.Parameter(torch.zeros(d, d), requires_grad=True)
        nn.init.normal_(self.W, std=0.1)


_UNSUPPORTED_FLAGS = ('use_attn_affinity', 'use_corr_affinity')
_REFINE_FLAGS = ('use_lgr', 'use_ransac', 'use_ratio_test', 'threshold_corr', 'remove_outliers_overlap',
                 'use_overlap_as_weights', 'remove_points_from_val')


from ._concurrency import no_side_stream   # noqa: F401  (re-exported: streams.py, tests, bench.py)


def _meta_tensors(meta):
    for v in meta.values():
        # list.__iter__: the index lists convert to int64 when iterated through their own __iter__
        items = v.values() if isinstance(v, dict) else (list.__iter__(v) if isinstance(v, list) else ())
        for t in items:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                yield t


class EncodedClouds:
    """What RegTR.encode leaves of a list of clouds and RegTR.register reads: the projected superpoint tokens and the
    coarsest-level points, both packed cloud after cloud, with the per-cloud superpoint counts on the host (`lens`)
    and as a device prefix (`cu`), plus the kpconv_meta of the encode call (None once encodings were concatenated)."""

    def __init__(self, tokens, points, lens, cu=None, kpconv_meta=None):
        lens = [int(n) for n in lens]
        if tokens.shape[0] != sum(lens) or points.shape[0] != sum(lens):
            raise ValueError(f"EncodedClouds: {tokens.shape[0]} token rows, {points.shape[0]} points, counts sum to {sum(lens)}")
        self.tokens, self.points, self.lens = tokens, points, lens
        self.cu = cu if cu is not None else ops.lengths_to_cu(lens, tokens.device)
        self.kpconv_meta = kpconv_meta

    def __len__(self):
        return len(self.lens)

    def _check(self, i):
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < len(self.lens):
            raise ValueError(f"cloud index {i!r} is not an index in range({len(self.lens)})")
        return int(i)

    def select(self, indices):
        """The encodings of clouds `indices` (any order, repeats allowed): host bookkeeping and one concatenation of
        row ranges per tensor.  The pyramid metadata describes the whole encode call and stays with it."""
        indices = [self._check(i) for i in indices]
        if not indices:
            raise ValueError("select: empty index list")
        start = np.concatenate([[0], np.cumsum(self.lens)])
        rows = [slice(int(start[i]), int(start[i + 1])) for i in indices]
        return EncodedClouds(torch.cat([self.tokens[r] for r in rows]), torch.cat([self.points[r] for r in rows]),
                             [self.lens[i] for i in indices])

    @staticmethod
    def cat(encodings):
        """Several encodings as one (a sequence keeps frame t and appends frame t+1): one concatenation per tensor.
        kpconv_meta does not survive: it describes one encode call."""
        encodings = list(encodings)
        if not encodings:
            raise ValueError("cat: empty list of encodings")
        return EncodedClouds(torch.cat([e.tokens for e in encodings]), torch.cat([e.points for e in encodings]),
                             [n for e in encodings for n in e.lens])


def check_point_feats(in_dim: int, clouds, feats, names):
    """Per-point input features of an encode call, checked on the host: `feats` is None (then cfg.in_feats_dim must
    be 1: the encoder runs on a column of ones) or one [n_i, in_dim] float32 tensor per cloud, row-aligned with it and
    on its device.  names[i] says which pair or cloud entry i is, for the message.  Returns the list (or None)."""
    in_dim = int(in_dim)
    if feats is None:
        if in_dim != 1:
            raise ValueError(f"cfg.in_feats_dim = {in_dim}: the batch must carry per-point input features "
                             f"('src_point_feats' / 'tgt_point_feats', 'cloud_point_feats' or encode(point_feats=...)), "
                             f"one [n, {in_dim}] float32 tensor per cloud")
        return None
    feats = list(feats)
    if len(feats) != len(clouds):
        raise ValueError(f"point features: {len(feats)} entries for {len(clouds)} clouds")
    for c, f, name in zip(clouds, feats, names):
        if not isinstance(f, torch.Tensor) or f.dim() != 2 or int(f.shape[1]) != in_dim:
            shape = tuple(f.shape) if isinstance(f, torch.Tensor) else type(f).__name__
            raise ValueError(f"point features of {name}: expected [n, {in_dim}] (cfg.in_feats_dim), got {shape}")
        if int(f.shape[0]) != int(c.shape[0]):
            raise ValueError(f"point features of {name}: {int(f.shape[0])} rows for a cloud of {int(c.shape[0])} points")
        if f.dtype != torch.float32:
            raise ValueError(f"point features of {name}: dtype {f.dtype}, expected torch.float32")
        if f.device != c.device:
            raise ValueError(f"point features of {name}: on {f.device}, its cloud is on {c.device}")
    return feats


def batch_point_feats(in_dim: int, batch, shared=None):
    """The input features of a batch in _encode's cloud order -- [src_0.., tgt_0..] of 'src_point_feats' /
    'tgt_point_feats' on pair lists, 'cloud_point_feats' of a clouds-and-pairs batch -- or None; raises ValueError
    (check_point_feats) on the host."""
    if shared is not None:
        clouds = shared[0]
        return check_point_feats(in_dim, clouds, batch.get('cloud_point_feats'),
                                 [f"clouds[{i}]" for i in range(len(clouds))])
    src, tgt = list(batch['src_xyz']), list(batch['tgt_xyz'])
    fs, ft = batch.get('src_point_feats'), batch.get('tgt_point_feats')
    if (fs is None) != (ft is None):
        raise ValueError("point features: 'src_point_feats' and 'tgt_point_feats' come together")
    names = [f"the source of pair {b}" for b in range(len(src))] + [f"the target of pair {b}" for b in range(len(tgt))]
    return check_point_feats(in_dim, src + tgt, None if fs is None else list(fs) + list(ft), names)


class RegTR(nn.Module):
    def __init__(self, cfg, *args, compute_upsamples=True, order=ops.ORDER_REFERENCE,
                 return_attn=False, record_attn=False, **kwargs):
        super().__init__()
        self.cfg = cfg
        self.return_attn = return_attn
        # True = the caller guarantees that the input clouds are materialised in device memory when
        # forward() is called (not the product of work still queued on the current stream): the
        # pyramid of this call may then start on the side stream while the previous call's
        # transformer / matching tail is still running on the caller's stream.  Default False:
        # the side stream first waits for everything queued on the caller's stream.
        self.inputs_resident = False
        for flag in _UNSUPPORTED_FLAGS:
            if cfg.get(flag, False):
                raise NotImplementedError(f"cfg.{flag}=True is not supported (use_attn_affinity raises "
                                          "ValueError in the reference itself, qk_regtr_full.py:505-511)")
        if cfg.get('pos_emb_type', 'sine') not in ('sine', 'learned'):
            raise NotImplementedError("pos_emb_type must be 'sine' or 'learned' (qk_regtr_full.py:52-58)")
        if cfg.get('neighbor_select', 'nearest') not in NEIGHBOR_SELECT:
            raise NotImplementedError("neighbor_select must be 'nearest' (the reference's CPU Preprocessor) or "
                                      "'index' (its PreprocessorGPU, kpconv.py:265-292)")

        self.preprocessor = Preprocessor(cfg, compute_upsamples=compute_upsamples, order=order,
                                         neighbor_select=cfg.get('neighbor_select', 'nearest'),
                                         tie_order=cfg.get('tie_order', 'index'))
        self.kpf_encoder = KPFEncoder(cfg, cfg.d_embed)
        self.feat_proj = nn.Linear(self.kpf_encoder.encoder_skip_dims[-1], cfg.d_embed, bias=True)
        if cfg.get('pos_emb_type', 'sine') == 'sine':
            self.pos_embed = PositionEmbeddingCoordsSine(3, cfg.d_embed,
                                                         scale=cfg.get('pos_emb_scaling', 1.0))
            self._pos_bound = 1.0                           # |sin|, |cos| <= 1
        else:
            self.pos_embed = PositionEmbeddingLearned(3, cfg.d_embed)
            # max |MLP(xyz)| depends on the coordinates: no static bound, the cross-encoder runs operator by operator
            self._pos_bound = None
        encoder_layer = TransformerCrossEncoderLayer(
            cfg.d_embed, cfg.nhead, cfg.d_feedforward, cfg.dropout,
            activation=cfg.transformer_act, normalize_before=cfg.pre_norm,
            sa_val_has_pos_emb=cfg.sa_val_has_pos_emb, ca_val_has_pos_emb=cfg.ca_val_has_pos_emb,
            attention_type=cfg.attention_type)
        encoder_norm = nn.LayerNorm(cfg.d_embed) if cfg.pre_norm else None
        self.transformer_encoder = TransformerCrossEncoder(encoder_layer, cfg.num_encoder_layers,
                                                           encoder_norm, return_intermediate=False)
        # opt-in: keep the cross-encoder's attention maps (transformer_encoder.get_attentions())
        self.transformer_encoder.record_attn = record_attn
        self.beta = nn.Parameter(torch.tensor(1.0))
        self.alpha = nn.Parameter(torch.tensor(1.0))
        self.overlap_predictor = nn.Linear(cfg.d_embed, 1)
        if cfg.get('feature_loss_type', 'infonce') == 'infonce':
            self.feature_criterion = _BilinearW(cfg.d_embed)
            self.feature_criterion_un = _BilinearW(cfg.d_embed)

    # ------------------------------------------------------------------ #
    def forward(self, batch):
        """model.train() + gradients enabled: differentiable (HIP backward, autograd.py).
        model.eval() (the reference's test loop, trainer.py:216-260) or torch.no_grad():
        the inference path -- fused in-projection, no tape, nothing saved.
        batch: `src_xyz` / `tgt_xyz` lists, or `clouds` and `pairs` (shared_clouds.py): every cloud is encoded once
        and used by any number of the batch's pairs, in training as well.
        Per-point input features (cfg.in_feats_dim columns: colour, intensity, height ...): `src_point_feats` /
        `tgt_point_feats`, lists of [n_i, C] float32 device tensors row-aligned with the clouds, or `cloud_point_feats`
        aligned with `clouds`.  Without them (in_feats_dim = 1 only) the encoder runs on a column of ones."""
        shared = None
        icp_refine = bool(self.cfg.get('icp_refine', False))
        if icp_refine and ('clouds' in batch or (self.training and torch.is_grad_enabled())):
            raise NotImplementedError("cfg.icp_refine polishes the pose of src_xyz / tgt_xyz batches in inference "
                                      "(model.eval() or torch.no_grad()): not in training, not over shared clouds")
        if 'clouds' in batch:
            shared = shared_clouds.check_batch(batch)       # raises on the host, before any launch
        feats = batch_point_feats(self.cfg.get('in_feats_dim', 1), batch, shared)   # likewise
        if not self.training and torch.is_grad_enabled():
            with torch.no_grad():
                out = self._forward(batch, shared, feats)
                return self._icp_polish(out, batch) if icp_refine else out
        if self.training and torch.is_grad_enabled():
            ops.prime_weight_ranges(self.parameters())      # one measuring launch for every weight the step moved
        out = self._forward(batch, shared, feats)
        return self._icp_polish(out, batch) if icp_refine else out

    def _icp_polish(self, out, batch):
        """cfg.icp_refine: ICP from the predicted pose on the input clouds, all pairs in one call -- point-to-point, or
        with cfg.icp_method = 'point_to_plane' point-to-plane on target normals estimated at cfg.icp_normals_radius;
        the network's pose stays in the output as 'pose_coarse'."""
        cfg = self.cfg
        dist = cfg.get('icp_distance', None)
        dist = 2.0 * float(cfg.first_subsampling_dl) if dist is None else float(dist)
        src, tgt = [c.to(torch.float32) for c in batch['src_xyz']], [c.to(torch.float32) for c in batch['tgt_xyz']]
        method = cfg.get('icp_method', 'point_to_point')
        if method == 'point_to_plane':
            from . import icp_plane
            radius = cfg.get('icp_normals_radius', None)
            radius = 2.5 * float(cfg.first_subsampling_dl) if radius is None else float(radius)
            r = icp_plane.icp_pairs(src, tgt, None, out['pose'], dist, int(cfg.get('icp_max_iter', 30)),
                                    kernel=cfg.get('icp_kernel', 'l2'), kernel_k=cfg.get('icp_kernel_k', None),
                                    normals_radius=radius)
        elif method == 'point_to_point':
            from . import icp
            r = icp.icp_pairs(src, tgt, out['pose'], dist, int(cfg.get('icp_max_iter', 30)))
        else:
            raise ValueError(f"cfg.icp_method {method!r}, expected 'point_to_point' or 'point_to_plane'")
        out['pose_coarse'] = out['pose']
        out['pose'], out['icp_fitness'], out['icp_rmse'] = r['pose'], r['fitness'], r['inlier_rmse']
        return out

    def _forward(self, batch, shared=None, feats=None):
        if shared is not None:
            return self._forward_shared(batch, *shared, feats=feats)
        B = len(batch['src_xyz'])
        tokens, xyz_c, lens_c, meta = self._encode(list(batch['src_xyz']) + list(batch['tgt_xyz']), feats)
        batch['kpconv_meta'] = meta                      # qk_regtr_full.py:153
        return self._register(tokens, xyz_c, lens_c[:B], lens_c[B:], pair_keys=batch.get('pair_key'))

    def _forward_shared(self, batch, clouds, src, tgt, feats=None):
        """forward() on a batch of clouds and pairs: _encode once over the clouds (on the tape when training), tokens
        and points laid out per pair by the pair gather (differentiable over the tokens; the points carry no
        gradient), then the unchanged _register.  Leaves in the batch what compute_loss, overlap.label_batch and
        training.compute_metrics read: the encode call's kpconv_meta, the per-pair views of the clouds as src_xyz /
        tgt_xyz (the cloud tensors themselves) and the pair layout under '_pair_layout'."""
        tokens, xyz_c, _, meta = self._encode(clouds, feats)
        batch['kpconv_meta'] = meta
        layout = shared_clouds.PairLayout(src, tgt, meta['_lens_host'], tokens.device)   # host lengths: no read-back
        batch['_pair_layout'] = layout
        batch['src_xyz'], batch['tgt_xyz'] = shared_clouds.pair_views(batch)
        P = len(src)
        cu = meta['_cu'][len(meta['points']) - 1]
        src_lens, tgt_lens = layout.seg_lens[-1][:P], layout.seg_lens[-1][P:]
        segments = make_segments(src_lens, tgt_lens, tokens.device)
        tok = shared_clouds.pair_gather(tokens, cu, layout)
        with torch.no_grad():
            xyz = shared_clouds.pair_gather(xyz_c, cu, layout)
        return self._register(tok, xyz, src_lens, tgt_lens, segments, batch.get('pair_key'))

    def _encode(self, clouds, feats=None):
        """The per-cloud half of the forward: pyramid, KPConv encoder, feat_proj.  Nothing here looks across clouds.
        feats: checked per-point input features, one [n_i, in_feats_dim] tensor per cloud, or None = a column of ones.
        Returns (tokens [sum L, d_embed], coarsest points [sum L, 3], host superpoint counts, kpconv_meta)."""
        # Pyramid (index work, never differentiated: qk_regtr_full.py:152) and KPConv encoder on a
        # column of ones (:157-166).  The pyramid is built on a SIDE stream and the blocks of a
        # level are launched on the caller's stream as soon as their part exists: the searches of
        # the deeper levels -- small latency-bound kernels, each followed by a device->host read of
        # a size -- run beside the big convolutions of the shallower ones instead of in front of
        # them (SPR_NO_SIDE_STREAM=1: one stream, pyramid first).
        device = clouds[0].device
        if feats is None:
            feats0 = torch.ones((sum(int(c.shape[0]) for c in clouds), 1), dtype=torch.float32, device=device)
        else:
            # level 0 is the input cloud: the features are never subsampled.  in_feats_dim 2..8 runs the first
            # KPConv on the small-Cin kernel (stem.few_shape_ok), wider input on the generic one
            feats0 = torch.cat(list(feats)).contiguous()
        if _concurrency.active(device):
            main = torch.cuda.current_stream(device)
            side = _concurrency.aux_stream(main, device, 'pyramid')
            if not self.inputs_resident:
                side.wait_stream(main)                   # the clouds were produced on the caller's stream

            def pyramid():
                gen = self.preprocessor.stream(clouds)
                while True:
                    with torch.no_grad(), torch.cuda.stream(side):
                        try:
                            item = next(gen)             # host blocks on the side stream's reads only
                        except StopIteration:
                            return
                        ev = torch.cuda.Event()
                        ev.record(side)
                    main.wait_event(ev)
                    yield item
            feats_un, _, meta = self.kpf_encoder.forward_streamed(feats0, pyramid())
            for t in _meta_tensors(meta):                # allocated on the side stream, read on this one
                t.record_stream(main)
        else:
            with torch.no_grad():
                meta = self.preprocessor(clouds)
            feats_un, _ = self.kpf_encoder(feats0, meta)
        tokens = ops.linear(feats_un, self.feat_proj.weight, self.feat_proj.bias)
        return tokens, meta['points'][-1], meta['_lens_host'][-1], meta

    def _register(self, tokens, xyz_c, src_lens, tgt_lens, segments=None, pair_keys=None):
        """The per-pair half: position embedding, cross-encoder, overlap head, matching + pose on tokens / points
        packed [src_0..src_{B-1}, tgt_0..tgt_{B-1}].  segments: make_segments(src_lens, tgt_lens) if the caller has it.
        pair_keys: what keys the RANSAC draws of use_ransac ([B] ints; None = the position in the batch)."""
        cfg = self.cfg
        B = len(src_lens)
        device = tokens.device

        # superpoint attention on packed tokens (qk_regtr_full.py:199-230)
        pe = self.pos_embed(xyz_c) if cfg.transformer_encoder_has_pos_emb else None
        cu, seg_self, seg_cross, max_len = segments if segments is not None else make_segments(src_lens, tgt_lens, device)
        seg_host = ([int(n) for n in list(src_lens) + list(tgt_lens)], list(range(2 * B)),
                    list(range(B, 2 * B)) + list(range(B)))
        cond = self.transformer_encoder.forward_packed(tokens, cu, seg_self, seg_cross, max_len, pos=pe,
                                                       seg_host=seg_host, pos_bound=self._pos_bound)

        # overlap head (qk_regtr_full.py:248-249)
        overlap = ops.linear(cond, self.overlap_predictor.weight, self.overlap_predictor.bias,
                             act=ops.ACT_SIGMOID)

        # matching + pose (qk_regtr_full.py:423-672), all pairs at once
        cu_host = [0]
        for n in list(src_lens) + list(tgt_lens):
            cu_host.append(cu_host[-1] + int(n))
        refine = any(cfg.get(f, False) for f in _REFINE_FLAGS)
        if refine and torch.is_grad_enabled() and self.training:
            raise NotImplementedError("the config-off refinements are inference-time options")
        val2 = None
        w = t_hat = None
        if (cfg.use_sinkhorn and not refine and bool(cfg.slack) and not torch.is_grad_enabled()):
            # inference: both heads read the same correlation matrices -- computed and stored once
            val, val2, ind, w, t_hat = ops.match_and_sinkhorn(cond, xyz_c, cu, cu_host, B, self.alpha, self.beta,
                                                              int(cfg.sinkhorn_itr),
                                                              top2=bool(cfg.get('use_ratio_test', False)))
        elif cfg.get('use_ratio_test', False):
            val, val2, ind = ops.match_dualsoftmax_top2(cond, cu, cu_host, B)
        else:
            val, ind = ops.match_dualsoftmax(cond, cu, cu_host, B)
        n_src = cu_host[B]
        src_xyz_all, tgt_xyz_all = xyz_c[:n_src], xyz_c[n_src:]
        refined = None
        if refine:
            refined = self._refined_pose(xyz_c, overlap, val, val2, ind, cu, cu_host, B, cond, pair_keys)
            pose = refined['pose']
        elif cfg.use_sinkhorn:
            if w is None:
                w, t_hat = ops.sinkhorn_correspondences(cond, xyz_c, cu, cu_host, B,
                                                        self.alpha, self.beta,   # device scalars, no sync
                                                        int(cfg.sinkhorn_itr), bool(cfg.slack))
            pose = ops.weighted_procrustes(src_xyz_all, t_hat, w, cu[:B + 1].contiguous())
        else:
            pose = self._pose_from_matches(xyz_c, val, ind, cu, cu_host, B)

        # ---- reference-shaped outputs (lists over the batch) ----
        def split(t, lens, off):
            out, o = [], off
            for n in lens:
                out.append(t[o:o + n])
                o += n
            return out

        src_feat = [f.unsqueeze(0) for f in split(cond, src_lens, 0)]
        tgt_feat = [f.unsqueeze(0) for f in split(cond, tgt_lens, n_src)]
        src_kp, tgt_kp = split(xyz_c, src_lens, 0), split(xyz_c, tgt_lens, n_src)
        src_ov = [o.unsqueeze(0) for o in split(overlap, src_lens, 0)]
        tgt_ov = [o.unsqueeze(0) for o in split(overlap, tgt_lens, n_src)]
        vals, inds, src_corr, tgt_corr = [], [], [], []
        ind_l = ind.long()                               # one conversion / one gather for all pairs
        matched_pts = None
        if not cfg.use_sinkhorn and refined is None:
            off, _, _, _ = self._match_index_arrays(cu_host, B, device)
            matched_pts = xyz_c[ind_l + off]             # partner point of every token
        for b in range(B):
            N, M = src_lens[b], tgt_lens[b]
            if N > M:   # one match per tgt point (qk_regtr_full.py:455-479)
                sl = slice(cu_host[B + b], cu_host[B + b + 1])
                v, i = val[sl], ind_l[sl]
                s_pts = src_kp[b] if matched_pts is None else matched_pts[sl]
                t_pts = tgt_kp[b]
            else:       # one match per src point (:563-588)
                sl = slice(cu_host[b], cu_host[b + 1])
                v, i = val[sl], ind_l[sl]
                s_pts = src_kp[b]
                t_pts = tgt_kp[b] if matched_pts is None else matched_pts[sl]
            if refined is not None:
                v, i, s_pts, t_pts = (refined[k][b] for k in ('val', 'ind', 'src_pts', 'tgt_pts'))
            vals.append(v)
            inds.append(i)
            src_corr.append(s_pts)
            tgt_corr.append(t_pts)

        attn = [None] * B
        if self.return_attn:
            attn = [self._dense_attn(src_feat[b][0], tgt_feat[b][0]) for b in range(B)]
        return {
            'pose': pose, 'attn': attn,
            'src_feat': src_feat, 'tgt_feat': tgt_feat,
            'src_kp': src_kp, 'tgt_kp': tgt_kp,
            'src_corr': src_corr, 'tgt_corr': tgt_corr,
            'src_overlap': src_ov, 'tgt_overlap': tgt_ov,
            'overlap_prob_list': vals, 'ind_list': inds,
        }

    # ------------------------------------------------------------------ #
    # Encode each cloud once, register any list of pairs over the encodings (inference only).
    def _inference_only(self, what):
        if self.training:
            raise RuntimeError(f"RegTR.{what} is an inference path: call model.eval() first (training goes through forward)")

    def encode(self, clouds, point_feats=None) -> EncodedClouds:
        """Pyramid, KPConv encoder and feat_proj of a list of [N_i, 3] float32 device clouds -- the part of forward()
        that never looks across clouds -- kept for any number of register() calls.  point_feats: per-point input
        features, one [N_i, cfg.in_feats_dim] float32 device tensor per cloud (None: a column of ones)."""
        self._inference_only("encode")
        clouds = list(clouds)
        if not clouds:
            raise ValueError("encode: empty cloud list")
        clouds = [ops._dev(c, f"clouds[{i}]", torch.float32) for i, c in enumerate(clouds)]   # CPU tensor: raises
        if any(c.dim() != 2 or c.shape[1] != 3 or c.shape[0] == 0 for c in clouds):
            raise ValueError("encode: every cloud must be a non-empty [N, 3] tensor")
        feats = check_point_feats(self.cfg.get('in_feats_dim', 1), clouds, point_feats,
                                  [f"clouds[{i}]" for i in range(len(clouds))])
        with torch.no_grad():
            tokens, xyz_c, lens_c, meta = self._encode(clouds, feats)
        return EncodedClouds(tokens, xyz_c, lens_c, cu=meta['_cu'][len(meta['points']) - 1], kpconv_meta=meta)

    def register(self, enc: EncodedClouds, pairs, pair_keys=None) -> dict:
        """forward()'s output dict for the pairs (src_index, tgt_index) into `enc`: one ops.pair_gather per tensor
        lays tokens and points out as [src_0..src_{P-1}, tgt_0..tgt_{P-1}], then the unchanged second half of
        forward() runs (position embedding of the gathered points, cross-encoder, overlap head, matching + pose).
        pair_keys: as batch['pair_key'] of forward() (the RANSAC draws of use_ransac; None = the position in `pairs`)."""
        self._inference_only("register")
        pairs = [tuple(p) for p in pairs]
        if not pairs:
            raise ValueError("register: empty pair list")
        if any(len(p) != 2 for p in pairs):
            raise ValueError("register: pairs are (src_index, tgt_index)")
        src = [enc._check(p[0]) for p in pairs]
        tgt = [enc._check(p[1]) for p in pairs]
        tokens = ops._dev(enc.tokens, "enc.tokens", torch.float32)
        points = ops._dev(enc.points, "enc.points", torch.float32)
        P = len(pairs)
        src_lens, tgt_lens = [enc.lens[i] for i in src], [enc.lens[i] for i in tgt]
        with torch.no_grad():
            segments = make_segments(src_lens, tgt_lens, tokens.device)      # cu_out from the host counts: no read-back
            idx = torch.from_numpy(np.asarray(src + tgt, dtype=np.int32)).to(tokens.device)
            rows = sum(src_lens) + sum(tgt_lens)
            tok = ops.pair_gather(tokens, enc.cu, idx[:P], idx[P:], segments[0], rows=rows)
            xyz = ops.pair_gather(points, enc.cu, idx[:P], idx[P:], segments[0], rows=rows)
            return self._register(tok, xyz, src_lens, tgt_lens, segments, pair_keys)

    # ------------------------------------------------------------------ #
    def compute_loss(self, pred, batch):
        """Forward of RegTR.compute_loss (qk_regtr_full.py:313-368): overlap BCE on the
        coarsest level of compute_overlaps, InfoNCE or circle feature loss (cfg.feature_loss_type)
        against the ground-truth transformed keypoints, L1 transform loss; total = T + 0.1 feature + overlap.
        batch needs 'pose' [B,3,4], 'src_overlap' / 'tgt_overlap' (per-point masks) and the
        'kpconv_meta' a forward left there.  Differentiable when `pred` came from a forward with
        gradients enabled: losses['total'].backward() then runs the HIP backward (autograd.py)."""
        cfg = self.cfg
        circle = cfg.get('feature_loss_type', 'infonce') == 'circle'
        if not circle and cfg.get('feature_loss_type', 'infonce') != 'infonce':
            raise NotImplementedError("feature_loss_type must be 'infonce' or 'circle' (qk_regtr_full.py:91-96)")
        if cfg.get('inlier_loss_on', False):
            raise NotImplementedError("inlier_loss_on is off in every shipped config")
        meta = batch['kpconv_meta']
        device = meta['points'][0].device
        B = len(batch['src_xyz'])
        pose_gt = batch['pose'].to(device=device, dtype=torch.float32).contiguous()

        # compute_overlaps (kpconv.py:552-578): average the per-point masks up the pyramid
        with torch.no_grad():   # ground-truth side: no gradient
            ov = torch.cat([o.to(device) for o in list(batch['src_overlap']) + list(batch['tgt_overlap'])]).float()
            layout = batch.get('_pair_layout') if 'clouds' in batch else None
            if layout is not None:   # a batch of clouds and pairs: the pools index the cloud layout, the masks are per pair
                pyr = shared_clouds.overlap_pyramid(ov, meta, layout)
                ov = pyr[f"pyr_{len(meta['points']) - 1}"]
            else:
                pyr = {'pyr_0': ov}
                for p in range(1, len(meta['points'])):
                    ov = ops.overlap_pool(ov, meta['_i32'][('pools', p - 1)], meta['points'][p - 1].shape[0])
                    pyr[f'pyr_{p}'] = ov
            batch['overlap_pyr'] = pyr

        # overlap loss: the (already sigmoided) predictions go through BCEWithLogits (:248, :329)
        pred_ov = torch.cat([o[0, :, 0] for o in list(pred['src_overlap']) + list(pred['tgt_overlap'])])
        losses = {'overlap': ops.bce_logits_mean(pred_ov.contiguous(), ov)}

        W = None if circle else self.feature_criterion.W
        feat, t_l1 = [], []
        # the reference overwrites `feature_loss` for every entry of feature_loss_on
        # (qk_regtr_full.py:340-345): only the LAST index contributes
        last = list(cfg.get('feature_loss_on', [0]))[-1:]
        if circle:   # CircleLossFull (qk_regtr_full.py:94-96): every pair in one batched call
            for i in last:
                feat = list(ops.circle_loss([s[i] for s in pred['src_feat']], [t[i] for t in pred['tgt_feat']],
                                            pred['src_kp'], pose_gt, pred['tgt_kp'], cfg.r_p, cfg.r_n))
        for b in range(B):
            for i in ([] if circle else last):
                feat.append(ops.infonce_pair(pred['src_feat'][b][i].contiguous(), pred['tgt_feat'][b][i].contiguous(),
                                             pred['src_kp'][b].contiguous(), pose_gt[b], pred['tgt_kp'][b].contiguous(),
                                             W, cfg.r_p, cfg.r_n))
            t_l1.append(ops.transform_l1_pair(pose_gt[b], pred['pose'][b].contiguous(), pred['src_kp'][b].contiguous()))
        if torch.is_grad_enabled() and any(t.requires_grad for t in feat + t_l1):
            losses['feature'] = torch.stack(feat).mean()                            # on the tape
            losses['T'] = torch.stack(t_l1).sum()
        else:
            losses['feature'] = ops.sum_scaled(torch.stack(feat), 1.0 / len(feat))  # mean over pairs (:314)
            losses['T'] = ops.sum_scaled(torch.stack(t_l1), 1.0)                    # sum over pairs (:353)
        losses['total'] = losses['T'] + 0.1 * losses['feature'] + losses['overlap']
        power = float(cfg.get('deform_fitting_power', 0.0))
        if power > 0:
            # KPConv's p2p_fitting_regularizer over the encoder's deformable blocks, from the forward that left
            # kpconv_meta: one term per encode call (per cloud on a batch of clouds and pairs, not per pair); on the
            # tape when that forward was, a plain value under no_grad.  None without a deformable block.
            from . import deform_reg
            terms = deform_reg.regularizer_terms(self.kpf_encoder, power, float(cfg.get('repulse_extent', 1.2)))
            if terms is not None:
                losses['deform_reg'], losses['deform_fit'], losses['deform_rep'] = terms
                losses['total'] = losses['total'] + losses['deform_reg']
        return losses

    def _refined_pose(self, xyz_c, overlap, val, val2, ind, cu, cu_host, B, cond, pair_keys=None):
        """The config-off refinements of RegTR.softmax_correlation (qk_regtr_full.py:445-668) for all pairs in ONE
        library call (ops.refine_pairs): Lowe ratio test (:370-384), median threshold (:471-473), overlap weighting
        (:484-494), top-k pruning (:499-502), then the pose, then LGR (:386-398).  With use_sinkhorn the Sinkhorn solve
        goes first and its pose stands (:525-536); RANSAC (:400-421) follows only when use_ransac, for all pairs in one
        ops.ransac_pairs call: cfg.ransac_itr (500) hypotheses of cfg.ransac_sample_size (100) entries per pair, drawn
        from (cfg.ransac_seed, pair key) -- pair_keys [B] ints, None = the position in the batch -- so a pair's pose
        is the same on every call.  The per-pair tensors returned are views of the packed outputs."""
        cfg = self.cfg
        on = lambda f: bool(cfg.get(f, False))
        sink, topk, lgr = bool(cfg.use_sinkhorn), on('remove_points_from_val'), on('use_lgr')
        n_src = [cu_host[b + 1] - cu_host[b] for b in range(B)]
        n_tgt = [cu_host[B + b + 1] - cu_host[B + b] for b in range(B)]
        if on('use_overlap_as_weights') and not on('remove_outliers_overlap') and not sink:
            raise ValueError("use_overlap_as_weights needs remove_outliers_overlap (as in the reference)")
        if sink and lgr and not topk and any(n != m for n, m in zip(n_src, n_tgt)):
            raise ValueError("use_lgr over the Sinkhorn point sets needs src and tgt clouds of equal length "
                             "(or remove_points_from_val), as in the reference")
        if sink and on('use_ransac') and not topk and any(n != m for n, m in zip(n_src, n_tgt)):
            raise ValueError("use_ransac over the Sinkhorn point sets needs src and tgt clouds of equal length "
                             "(or remove_points_from_val), as in the reference")
        sk_pose = None
        if sink:   # the Sinkhorn pose ignores the pruned correspondences (:525-536)
            w, t_hat = ops.sinkhorn_correspondences(cond, xyz_c, cu, cu_host, B, self.alpha, self.beta,
                                                    int(cfg.sinkhorn_itr), bool(cfg.slack))
            sk_pose = ops.weighted_procrustes(xyz_c[:cu_host[B]], t_hat, w, cu[:B + 1].contiguous())
        k = [int(cfg.val_threshold * min(n, m)) for n, m in zip(n_src, n_tgt)] if topk else None
        r = ops.refine_pairs(val, val2, ind, overlap, xyz_c, cu, cu_host, B, k,
                             ratio=on('use_ratio_test'), median=on('threshold_corr'),
                             overlap_prune=on('remove_outliers_overlap'),
                             overlap_as_weights=on('use_overlap_as_weights') and on('remove_outliers_overlap'),
                             lgr_steps=int(cfg.num_refinement_steps) if lgr else 0,
                             lowe_thres=float(cfg.lowe_thres) if on('use_ratio_test') else 0.0,
                             acceptance_radius=float(cfg.acceptance_radius) if lgr else 0.0,
                             pose_in=sk_pose, sinkhorn=sink)
        oc = r['out_cu']
        out = {k_: [r[k_][oc[b]:oc[b + 1]] for b in range(B)] for k_ in ('val', 'ind', 'src_pts', 'tgt_pts')}
        if sink and not topk:      # the unpruned Sinkhorn sets are the clouds themselves
            out['src_pts'] = [xyz_c[cu_host[b]:cu_host[b + 1]] for b in range(B)]
            out['tgt_pts'] = [xyz_c[cu_host[B + b]:cu_host[B + b + 1]] for b in range(B)]
        out['pose'] = r['pose']
        if on('use_ransac'):   # all pairs in one call, over the packed sets refine_pairs left on the device
            a, bb = r['src_pts'], r['tgt_pts']
            if sink and not topk:  # the clouds themselves: with equal lengths they are packed by out_cu already
                a, bb = xyz_c[:cu_host[B]], xyz_c[cu_host[B]:]
            out['pose'] = ops.ransac_pairs(a, bb, r['val'], r['out_cu_dev'], oc, n_hyp=int(cfg.get('ransac_itr', 500)),
                                           sample=int(cfg.get('ransac_sample_size', 100)),
                                           seed=int(cfg.get('ransac_seed', 0)), pair_keys=pair_keys)['pose']
        return out

    @staticmethod
    def _ransac(src, tgt, weights, itr: int = 500, sample_size: int = 100, generator=None):
        """qk_regtr_full.py:400-421 (500 random 100-point subsets with replacement, keep the
        hypothesis with the lowest mean residual over ALL correspondences) as two launches."""
        n = src.shape[0]
        idx = torch.randint(0, n, (itr, sample_size), device=src.device, generator=generator).reshape(-1)
        set_cu = torch.arange(itr + 1, dtype=torch.int32, device=src.device) * sample_size
        poses = ops.weighted_procrustes(src[idx].contiguous(), tgt[idx].contiguous(), weights[idx].contiguous(), set_cu)
        score = ops.pose_scores(poses, src, tgt)
        return poses[torch.argmin(score)]          # first minimum, like the reference's strict '<'

    @staticmethod
    def _match_index_arrays(cu_host, B, device):
        """Index bookkeeping of the arg-max matches for ALL pairs, built once on the host and
        uploaded in one copy (the per-pair device ops it replaces were 3 tiny kernels per pair):
          off   [T]  what turns a token's match index (local to the partner cloud) into a global
                     token index: tgt start of the pair for src tokens, src start for tgt tokens;
          own   [S]  the tokens that carry a pair's matches: the tgt tokens when N_b > M_b, else the
                     src tokens (qk_regtr_full.py:455-479, :563-588);
          on_tgt[S]  1 where `own` is a tgt token;   set_cu [B+1]  prefix of the per-pair counts."""
        cu = np.asarray(cu_host, dtype=np.int64)
        n = cu[1:B + 1] - cu[:B]
        m = cu[B + 1:2 * B + 1] - cu[B:2 * B]
        off = np.concatenate([np.repeat(cu[B:2 * B], n), np.repeat(cu[:B], m)])
        on_tgt_pair = n > m
        starts = np.where(on_tgt_pair, cu[B:2 * B], cu[:B])
        counts = np.where(on_tgt_pair, m, n)
        set_cu = np.concatenate([[0], np.cumsum(counts)])
        own = np.repeat(starts - set_cu[:-1], counts) + np.arange(set_cu[-1])
        flag = np.repeat(on_tgt_pair.astype(np.int64), counts)
        packed = torch.from_numpy(np.concatenate([off, own, flag, set_cu])).to(device)
        T, S = off.shape[0], own.shape[0]
        return packed[:T], packed[T:T + S], packed[T + S:T + 2 * S].bool(), packed[T + 2 * S:].to(torch.int32)

    def _pose_from_matches(self, xyz_c, val, ind, cu, cu_host, B):
        """arg-max correspondences -> weighted Procrustes for all pairs in one
        launch.  For pair b the matched set lives on the tgt tokens when
        N_b > M_b and on the src tokens otherwise; build packed (a, b, w) by
        index arithmetic on the device."""
        off, own, on_tgt, set_cu = self._match_index_arrays(cu_host, B, xyz_c.device)
        matched = (ind.long() + off)[own]                  # global index of every match
        a_idx = torch.where(on_tgt, matched, own)          # src side
        b_idx = torch.where(on_tgt, own, matched)          # tgt side
        a = ops.gather_rows(xyz_c, a_idx.to(torch.int32))
        bb = ops.gather_rows(xyz_c, b_idx.to(torch.int32))
        w = val[own]
        return ops.weighted_procrustes(a, bb, w, set_cu)

    @staticmethod
    def _dense_attn(fs, ft):
        """Optional dense dual-softmax matrix for analysis (qk_regtr_full.py:453-459):
        correlation GEMM on the library, the two softmaxes as tensor ops."""
        corr = ops.linear(fs, ft) / (fs.shape[1] ** 0.5)
        return (torch.softmax(corr, dim=0) * torch.softmax(corr, dim=1)).unsqueeze(0)
