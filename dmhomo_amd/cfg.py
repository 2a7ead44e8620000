"""Conditional UNet + GaussianDiffusion with classifier-free guidance on MI355X.

Host-side mirror of the reference's
``DGM/denoising_diffusion_models/classifier_free_guidance.py`` (tag CFG): same class
names, constructor signatures, method names, ``state_dict`` keys and RNG call order,
so scripts written against the reference (``DGM/dgm_sample.py:28-38``) run
unchanged — but every tensor value is produced by the gfx950 kernels of
libdmhomo_hip.so (see ``engine.py``).  There is no CPU path.
"""
import torch
from torch import nn

from . import _params as P
from . import ops
from .engine import UnetEngine
from .sampling import DeviceRng, ModelPrediction, ScheduleHost, default, exists, extract  # noqa: F401
from .schedule import make_buffers, ddim_pairs, start_entry, linear_beta_schedule, cosine_beta_schedule  # noqa: F401


class Unet(nn.Module):
    """CFG:302-466.  ``forward`` launches the HIP program; parameters live in holders."""

    def __init__(self, dim, num_classes, cond_drop_prob=0.5, init_dim=None, out_dim=None, dim_mults=(1, 2, 4, 8),
                 channels=3, resnet_block_groups=8, learned_variance=False, learned_sinusoidal_cond=False,
                 random_fourier_features=False, learned_sinusoidal_dim=16):
        super().__init__()
        self.cond_drop_prob = cond_drop_prob
        self.channels = channels
        input_channels = channels + 3                       # rgb_flow * mask is concatenated, CFG:330,430
        init_dim = default(init_dim, dim)
        self.init_conv = nn.Conv2d(input_channels, init_dim, 7, padding=3)
        time_dim = dim * 4
        self.random_or_learned_sinusoidal_cond = learned_sinusoidal_cond or random_fourier_features
        # (GaussianDiffusion refuses such a model — CFG:514-515 — so it serves bare Unet.forward callers only)
        pos_emb, fourier_dim = P.time_embedding(dim, learned_sinusoidal_cond, random_fourier_features, learned_sinusoidal_dim)
        self.time_mlp = nn.Sequential(pos_emb, nn.Linear(fourier_dim, time_dim), nn.GELU(), nn.Linear(time_dim, time_dim))
        self.classes_emb = nn.Embedding(num_classes, dim)
        self.null_classes_emb = nn.Parameter(torch.randn(dim))
        classes_dim = dim * 4
        self.classes_mlp = nn.Sequential(nn.Linear(dim, classes_dim), nn.GELU(), nn.Linear(classes_dim, classes_dim))
        self.out_dim = default(out_dim, channels * (1 if not learned_variance else 2))
        P.build_trunk(self, dim, init_dim, dim_mults, input_channels, time_dim + classes_dim, resnet_block_groups,
                      self.out_dim, P.downsample_cfg)
        self.rng = DeviceRng()
        self._engine = UnetEngine(self, groups=resnet_block_groups)

    # ---- class-dropout draw of CFG:421-425 / prob_mask_like CFG:84-90
    def _keep_mask(self, batch, cond_drop_prob, device):
        if not cond_drop_prob > 0:
            return None
        prob = 1 - cond_drop_prob
        if prob == 1:
            return None                                      # keep every row
        if prob == 0:
            return self._null_mask(batch, device)
        if type(self.rng) is DeviceRng and self.rng.keyed:           # draw + compare + uint8 in one launch
            return ops.rng_keep_mask(self.rng.ids_for(batch), self.rng.state, prob)
        return (self.rng.uniform(batch, device) < prob).to(torch.uint8)

    def _null_mask(self, batch, device):
        """(batch,) uint8 zeros: every class dropped (the null pass, CFG:409) — one buffer per (batch, device), allocated once,
        never written and never replaced: a captured denoise step holds its address for as long as the graph lives"""
        cache = self.__dict__.setdefault('_null_keep', {})
        key = (int(batch), str(torch.device(device)))
        z = cache.get(key)
        if z is None:
            z = cache[key] = torch.zeros((batch,), device=device, dtype=torch.uint8)
        return z

    def _stem(self, x, rgb_flow, mask):
        """cat((x, rgb_flow*mask)) -> NHWC -> init_conv: identical for the cond and the null pass (CFG:430-432)."""
        if not x.is_cuda:
            raise RuntimeError('dmhomo_amd.Unet runs on the GPU only (HIP kernels); move the inputs with .cuda()')
        eng = self._engine
        eng.ensure_prepared()
        xin = ops.assemble_input(x.to(torch.float32).contiguous(), rgb_flow.to(torch.float32).contiguous(),
                                 mask.to(torch.float32).contiguous(), reps=1, cpad=eng.cin_pad)
        return eng.stem(xin)

    def _run(self, x, time, classes, rgb_flow, mask, keeps, taps=None, x0=None, first=None, out=None, rows=None,
             x0_per_pass=False, pert_lo=None):
        """rows [rep*B + b]: sample b under class-keep mask keeps[rep] -> (len(keeps)*B, out_dim, H, W).
        first: engine.first_conv(x0) when the caller shares it between passes.
        rows: ``ops.rows_from_keep`` list of the rows to compute (the others stay unwritten), or None for all.
        x0_per_pass: x0 holds the stem output of every pass already, len(keeps) * B rows (_cond_null_noflow).
        pert_lo: the rows >= pert_lo run mid_attn with the identity attention map (_cond_null_pag), or None for none."""
        eng = self._engine
        if x0 is None:
            x0 = self._stem(x, rgb_flow, mask)
        if len(keeps) > 1 and not x0_per_pass:
            x0 = x0.repeat(len(keeps), 1, 1, 1)              # row copies of the shared stem output
        time = time.to(torch.int64).contiguous()
        classes = classes.to(torch.int64).contiguous()
        tab = self.__dict__.get('_ss_tab')
        if tab is not None:
            # a replayed denoise step (GaussianDiffusion._sample_graphed): the (scale, shift) rows of every ResnetBlock come
            # from tables indexed by the step cursor and the row's class / keep bit — one small launch per pass instead of the
            # two embeddings, four small linears and the 512 -> 8 k linear at its head; bitwise the same rows (UnetEngine.ss_tables)
            T, Ct, cursor = tab
            B = classes.shape[0]
            ss_all = torch.empty((len(keeps) * B, T.shape[1]), device=T.device, dtype=torch.float32)
            for r, k in enumerate(keeps):
                ops.ss_gather(T, Ct, eng.mlp_b, cursor, classes, k, out=ss_all[r * B:(r + 1) * B])
            return eng.trunk(x0, None, taps, first=first, out=out, ss_all=ss_all, rows=rows, pert_lo=pert_lo)
        cond = eng.embed(time, [(classes, k) for k in keeps], len(keeps))
        return eng.trunk(x0, cond, taps, first=first, out=out, rows=rows, pert_lo=pert_lo)

    def forward(self, x, time, classes, rgb_flow, mask, cond_drop_prob=None):
        cond_drop_prob = default(cond_drop_prob, self.cond_drop_prob)
        keep = self._keep_mask(x.shape[0], cond_drop_prob, x.device)
        return self._run(x, time, classes, rgb_flow, mask, [keep])

    # 'batched': cond + null rows as ONE 2B launch sequence.  'streams': the two passes as two B-row
    # sequences on two HIP streams, so one pass's HBM-bound kernels and kernel tails overlap the other's
    # matrix-bound kernels.  Results are identical (rows are independent, tests pin that bitwise).
    cfg_mode = 'batched'
    stream_splits = 1      # 'streams' mode: row sub-batches per pass, each on its own stream

    def _cond_null(self, x, time, classes, rgb_flow, mask, gate=None):
        """the two passes of CFG:404,409: (cond logits, null logits, computed).  computed is None — every row of the cond
        logits was computed — or, with ``dedup_dropped_rows``, the (B,) uint8 class-keep mask: rows where it is 0 were left
        UNWRITTEN in the cond logits and equal the null logits' rows (``ops.sampler_step(..., keep=computed)``).
        gate: None, or the (cursor, guided) device tables of a replayed step under ``guidance_interval``: every pass then takes
        a row list from ``ops.rows_gated`` — at an unguided entry all B conditional rows are computed and no null row; the caller
        puts ``ops.guidance_gate`` behind the network."""
        B = x.shape[0]
        keep = self._keep_mask(B, self.cond_drop_prob, x.device)
        null = self._null_mask(B, x.device)
        dedup = bool(self.dedup_dropped_rows) and keep is not None
        if self.cfg_mode == 'streams':
            nsub = max(1, min(int(self.stream_splits), B))       # row sub-batches per pass (each on its own stream)
            nstreams = 2 * nsub
            if len(getattr(self, '_side', ())) != nstreams:
                self._side = tuple(torch.cuda.Stream(device=x.device) for _ in range(nstreams))
            cur = torch.cuda.current_stream()
            x0 = self._stem(x, rgb_flow, mask)                # once, on the main stream
            # ... and with it the first convolution behind it: the class embedding reaches a ResnetBlock only through the
            # scale / shift behind block1's GroupNorm, so downs.0.0.block1.proj(x0) is the same rows in both passes
            first = self._engine.first_conv(x0)
            cond_out = torch.empty((B, self.out_dim) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
            null_out = torch.empty_like(cond_out)
            bounds = [(i * B) // nsub for i in range(nsub + 1)]
            si = 0
            for k, dst, sub, null_side in ((keep, cond_out, dedup, False), (null, null_out, False, True)):
                for lo, hi in zip(bounds[:-1], bounds[1:]):
                    st = self._side[si]
                    si += 1
                    st.wait_stream(cur)
                    with torch.cuda.stream(st):
                        kk = None if k is None else k[lo:hi].contiguous()
                        fs = None if first is None else (first[0][lo:hi], first[1][lo:hi])
                        # (the pass writes its rows of the result itself: the fused final projection's destination)
                        if gate is not None:
                            rows = ops.rows_gated(kk if sub else None, hi - lo, 0, *gate, null_side=null_side)
                        else:
                            rows = ops.rows_from_keep(kk) if sub else None
                        self._run(None, time[lo:hi], classes[lo:hi], None, None, [kk], x0=x0[lo:hi], first=fs, out=dst[lo:hi],
                                  rows=rows)
            for st in self._side:
                cur.wait_stream(st)
            return cond_out, null_out, (keep if dedup else None)
        if gate is not None:
            rows = ops.rows_gated(keep if dedup else None, B, B, *gate)
        else:
            rows = ops.rows_from_keep(keep, extra=B) if dedup else None
        both = self._run(x, time, classes, rgb_flow, mask, [keep, null], rows=rows)
        return both[:B], both[B:], (keep if dedup else None)

    def _cond_null_noflow(self, x, time, classes, rgb_flow, mask, cond_scale):
        """the passes of GaussianDiffusion.flow_guidance (include/dmhomo_hip.h has the definition): (cond logits, null logits or
        None, no-flow logits, computed) as ONE launch sequence.  cond_scale != 1: 3B rows [c; n; u] — the two passes of
        _cond_null and the null class on a stem input whose three condition channels are +0.0 — with computed as _cond_null
        returns it.  cond_scale == 1: 2B rows [c; u] — forward's single pass and the SAME keep bits without the flow — with null
        and computed None.  The keep mask is drawn once, where _cond_null / forward draw it; every row is bitwise the row of a
        separate pass (rows are independent of their batch)."""
        if self.cfg_mode == 'streams':
            raise ValueError("flow_guidance with cfg_mode = 'streams': the third pass is defined for cfg_mode = 'batched' only")
        B, eng = x.shape[0], self._engine
        keep = self._keep_mask(B, self.cond_drop_prob, x.device)
        x0 = self._stem(x, rgb_flow, mask)
        # the no-flow stem input: assemble_input pads with zeros, so without a condition the three channels are +0.0
        x0u = eng.stem(ops.assemble_input(x.to(torch.float32).contiguous(), None, None, cpad=eng.cin_pad))
        if cond_scale == 1:
            both = self._run(None, time, classes, None, None, [keep, keep], x0=torch.cat((x0, x0u)), x0_per_pass=True)
            return both[:B], None, both[B:], None
        null = self._null_mask(B, x.device)
        dedup = bool(self.dedup_dropped_rows) and keep is not None
        rows = ops.rows_from_keep(keep, extra=2 * B) if dedup else None
        three = self._run(None, time, classes, None, None, [keep, null, null], x0=torch.cat((x0, x0, x0u)), rows=rows,
                          x0_per_pass=True)
        return three[:B], three[B:2 * B], three[2 * B:], (keep if dedup else None)

    def _cond_null_pag(self, x, time, classes, rgb_flow, mask, cond_scale):
        """the passes of GaussianDiffusion.pag_scale (include/dmhomo_hip.h has the definition): (cond logits, null logits or
        None, perturbed logits, computed) as ONE launch sequence.  cond_scale != 1: 3B rows [c; n; p] — the two passes of
        _cond_null and the conditional pass again with mid_attn's attention map replaced by the identity (pert_lo = 2B) — with
        computed as _cond_null returns it; under dedup_dropped_rows every perturbed row is computed.  cond_scale == 1: 2B rows
        [c; p] (pert_lo = B) with null and computed None.  The keep mask is drawn once, where _cond_null / forward draw it, and
        serves c and p; the stem output is shared (row copies); every row is bitwise the row of a separate pass."""
        if self.cfg_mode == 'streams':
            raise ValueError("pag_scale with cfg_mode = 'streams': the perturbed pass is defined for cfg_mode = 'batched' only")
        B = x.shape[0]
        keep = self._keep_mask(B, self.cond_drop_prob, x.device)
        if cond_scale == 1:
            both = self._run(x, time, classes, rgb_flow, mask, [keep, keep], pert_lo=B)
            return both[:B], None, both[B:], None
        null = self._null_mask(B, x.device)
        dedup = bool(self.dedup_dropped_rows) and keep is not None
        rows = ops.rows_from_keep(keep, extra=2 * B) if dedup else None
        three = self._run(x, time, classes, rgb_flow, mask, [keep, null, keep], rows=rows, pert_lo=2 * B)
        return three[:B], three[B:2 * B], three[2 * B:], (keep if dedup else None)

    # OPT-IN, off by default (bench.py's headline keeps it off and reports it under "variants").  The reference's conditional
    # pass draws a class-dropout mask with p = 0.5 (CFG:404 -> CFG:415,422), also while sampling: a dropped row of that pass
    # has exactly the inputs of the same sample's row in the null pass, so its logits equal the null logits and the guided
    # output is the null output.  With this switch those duplicate rows are not computed: the mask never leaves the device —
    # ``ops.rows_from_keep`` turns it into the list of active rows that every launch of the conditional pass takes
    # (include/dmhomo_hip.h, "Row subsets": the captured B-row grid stays, workgroups of inactive rows retire at once), and the
    # sampler step reads the null logits where the mask is 0.  B + (kept rows) UNet rows per step instead of 2B, the result
    # bit for bit the same (rows are independent of their batch — tests pin that), in every cfg_mode and under hip_graph.
    dedup_dropped_rows = False

    def forward_with_cond_scale(self, *args, cond_scale=1., **kwargs):
        """CFG:403-410: ``forward(*args, **kwargs)``; for cond_scale != 1 blended with ``forward(*args, cond_drop_prob=1.,
        **kwargs)`` — so, as in the reference, a caller's own ``cond_drop_prob`` is accepted only with cond_scale == 1."""
        if cond_scale == 1:
            return self.forward(*args, **kwargs)
        if 'cond_drop_prob' in kwargs or len(args) > 5:
            raise TypeError("forward() got multiple values for keyword argument 'cond_drop_prob'")   # as CFG:409 would
        x, time, classes, rgb_flow, mask = _bind_forward(self.forward, args, kwargs)
        logits, null, computed = self._cond_null(x, time, classes, rgb_flow, mask)
        out, _, _ = ops.sampler_step(ScheduleHost._blend_step(cond_scale), logits, null, null, None, want_x_start=False,
                                     keep=computed)
        return out


def _bind_forward(forward, args, kwargs):
    import inspect
    ba = inspect.signature(forward).bind(*args, **kwargs)           # TypeError for missing / unknown arguments, like a call
    a = ba.arguments
    return a['x'], a['time'], a['classes'], a['rgb_flow'], a['mask']


class GaussianDiffusion(nn.Module, ScheduleHost):
    """CFG:498-842 — sampling side on the GPU kernels; buffers and their names as the reference."""

    def __init__(self, model, *, image_size, timesteps=1000, sampling_timesteps=None, loss_type='l1',
                 objective='pred_noise', beta_schedule='cosine', p2_loss_weight_gamma=0., p2_loss_weight_k=1,
                 ddim_sampling_eta=1.):
        super().__init__()
        self._init_diffusion(model, image_size, timesteps, sampling_timesteps, loss_type, objective, beta_schedule,
                             p2_loss_weight_gamma, p2_loss_weight_k, ddim_sampling_eta)

    @property
    def rng(self):
        return self.model.rng

    @rng.setter
    def rng(self, value):
        self.model.rng = value

    # OPT-IN, None by default (every existing result, launch and graph key stays what it is).  apg_eta in [0, 1]: adaptive projected
    # guidance (Sadat, Hilliges, Weber 2024, "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion Models",
    # Algorithm 1; the reference has none) in sample(): per sample and step the update d = cond - null is split into its parts
    # parallel and orthogonal to the conditional logits and the guided logits are cond + (cond_scale - 1) * s * (d_orth + apg_eta *
    # d_par) — the paper attributes the saturation at high scales to the parallel part; 0 drops it, 1 keeps it (the usual blend in
    # exact arithmetic, not bit for bit: None is "off").  apg_norm_threshold > 0 caps the update's norm per sample, s = min(1,
    # threshold / |d|); apg_momentum in (-1, 1) replaces d by the running average d + momentum * (the previous step's average), zero
    # at the start of every loop (the paper's values at cond_scale 10-15 are eta 0, threshold 2.5-15 at its latent sizes, momentum
    # -0.5; the norm grows with sqrt(C * H * W)).  The definition is in include/dmhomo_hip.h; the coefficients come from fp64 row
    # sums (dmh_apg_coef), the guided logits (dmh_apg_apply) go through the existing step and threshold kernels as a conditional
    # output without a null pass, so both samplers and both clip modes take it.  It acts only where the network returns a null
    # pass (cond_scale != 1).  Refused together with guidance_rescale > 0 (the paper offers APG in its place) and with
    # guidance_interval (the running average across unguided entries has no definition yet).  model_predictions and
    # forward_with_cond_scale do not know it.  What it does to samples of trained weights has not been measured.
    apg_eta = None
    apg_norm_threshold = 0.
    apg_momentum = 0.

    def _check_apg(self):
        """-> None (off), or (eta, norm threshold, momentum) as floats"""
        num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
        eta, rho, beta = self.apg_eta, self.apg_norm_threshold, self.apg_momentum
        if eta is not None and not (num(eta) and 0. <= eta <= 1.):
            raise ValueError(f'apg_eta = {eta!r}: None (off), or a number in [0, 1]')
        if not (num(rho) and 0. <= rho < float('inf')):
            raise ValueError(f'apg_norm_threshold = {rho!r}: a finite number >= 0 (0: no threshold)')
        if not (num(beta) and -1. < beta < 1.):
            raise ValueError(f'apg_momentum = {beta!r}: a number in (-1, 1)')
        if eta is None:
            return None
        if self._check_guidance_rescale() > 0.:
            raise ValueError(f'apg_eta = {eta!r} together with guidance_rescale = {self.guidance_rescale!r}: adaptive projected '
                             f'guidance stands in place of the rescale, the two are not combined')
        if self._check_guidance_interval() is not None:
            raise ValueError(f'apg_eta = {eta!r} together with guidance_interval = {self.guidance_interval!r}: the running average '
                             f'across unguided entries is not defined')
        return float(eta), float(rho), float(beta)

    def _apg_on(self, cond_scale):
        """(eta, rho, beta) where the loop projects its guidance (apg_eta set and a null pass to project against: cond_scale !=
        1), else None: the calls as they were"""
        apg = self._check_apg()
        return apg if cond_scale != 1 else None

    @staticmethod
    def _apg_state(img, apg):
        """the buffers one eager loop keeps: the fp64 workspace, the guided logits and — with momentum — the running average,
        zero at the start of the loop"""
        return {'ws': ops.apg_workspace(img), 'guided': torch.empty_like(img),
                'run': torch.zeros_like(img) if apg[2] != 0. else None}

    @staticmethod
    def _apg_logits(step, cond, null, computed, apg, ast):
        """one eager step's guided logits: the coefficients, then the apply -> (guided, coef (B, 2)); the update behind it takes
        (guided, None, keep=None)"""
        eta, rho, beta = apg
        coef = ops.apg_coef(step, cond, null, eta, rho, beta, keep=computed, run=ast['run'], ws=ast['ws'])
        return ops.apg_apply(cond, null, coef, keep=computed, run=ast['run'], out=ast['guided']), coef

    # OPT-IN, None by default (every existing result, launch and graph key stays what it is).  photo_guidance = w in (0, 1]:
    # photometric-consistency guidance in sample() — training adds alpha_bar_t * mean(mask * l(flow_warp(im2, flow) - im1)) to the
    # loss (CFG:782-806), the reference's sampler ignores flow and mask beyond the stem.  With the switch on, at every entry of the
    # time list the blended x_start prediction is moved down the gradient of that term's squared form, E = mean(mask *
    # (flow_warp(im2, flow) - im1) ** 2): im1 towards the warped im2, im2 the transposed way, by lambda / 2 of the masked residual
    # with lambda = w * alpha_bar_t, the weight the loss gives the term; the im2 side is divided by max(1, s), s the mask-weighted
    # bilinear weight that lands on a pixel, which makes the step a descent of E for every flow (include/dmhomo_hip.h has the
    # definition and the argument).  The corrected logits (dmh_photo_guide) go through the existing step and threshold kernels as
    # a conditional output without a null pass, so both samplers, both clip modes, dedup_dropped_rows and both cfg_modes take it;
    # it needs no null pass and acts at cond_scale == 1 too.  Refused with another objective than pred_x0 (the logits are then
    # not the image pair), with guidance_rescale > 0 and apg_eta (they rescale / project the blend this step corrects: which goes
    # first has no definition yet) and with guidance_interval (the captured step would need the gate's null copy in front of the
    # correction).  model_predictions and forward_with_cond_scale do not know it.  ddpm.photometric_error gives E of any pair.
    # What it does to samples of trained weights has not been measured.
    photo_guidance = None

    def _check_photo_guidance(self):
        """-> None (off), or the weight w as a float"""
        w = self.photo_guidance
        if w is None:
            return None
        if not (isinstance(w, (int, float)) and not isinstance(w, bool) and 0. < w <= 1.):
            raise ValueError(f'photo_guidance = {w!r}: None (off), or a number in (0, 1]')
        if self.objective != 'pred_x0':
            raise ValueError(f'photo_guidance = {w!r} with objective = {self.objective!r}: the correction acts on the predicted '
                             f'image pair, which the network returns under pred_x0 only')
        if self._check_guidance_rescale() > 0.:
            raise ValueError(f'photo_guidance = {w!r} together with guidance_rescale = {self.guidance_rescale!r}: the rescale '
                             f'works on the blend that the correction replaces, the order of the two is not defined')
        if self.apg_eta is not None:
            raise ValueError(f'photo_guidance = {w!r} together with apg_eta = {self.apg_eta!r}: both hand guided logits to the '
                             f'step in place of the blend, the order of the two is not defined')
        if self._check_guidance_interval() is not None:
            raise ValueError(f'photo_guidance = {w!r} together with guidance_interval = {self.guidance_interval!r}: the '
                             f'correction is defined on the blend of every entry, not across unguided entries')
        return float(w)

    @staticmethod
    def _photo_state(shape, flow, mask, device):
        """the buffers one eager loop keeps: flow and mask as fp32, the preconditioner s (computed here, once per call), the
        zeroed fixed-point accumulator and the guided logits"""
        flow = flow.to(torch.float32).contiguous()
        mask = mask.to(torch.float32).contiguous()
        acc = ops.photo_acc(shape[0], shape[2], shape[3], device)
        return {'flow': flow, 'mask': mask, 'acc': acc, 's': ops.photo_weights(flow, mask, acc),
                'guided': torch.empty(shape, device=device, dtype=torch.float32)}

    def _photo_logits(self, step, cond, null, computed, w, pst, cond_scale, want_energy):
        """one eager step's corrected logits -> (guided, what the trace adds); the update behind it takes (guided, None,
        keep=None).  want_energy: E of the blend before the correction (two launches more, and the blend itself where there is
        a null pass: tracing only)"""
        more = {}
        if want_energy:
            blend = cond
            if null is not None:
                blend, _, _ = ops.sampler_step(self._blend_step(cond_scale), cond, null, null, None, want_x_start=False,
                                               keep=computed)
            more['photo'] = ops.photo_energy(blend, pst['flow'], pst['mask'])
        return ops.photo_guide(step, cond, null, computed, pst['flow'], pst['mask'], pst['s'], w, pst['acc'],
                               out=pst['guided']), more

    # ---- known pixels (sample_known; sampling.py: ScheduleHost.known_resample has the description, include/dmhomo_hip_known.h
    # the definition)
    KNOWN_MASKS = {'source': (0, 3), 'target': (3, 6)}

    def _known_inputs(self, known, known_mask, shape):
        """the checks of a sample_known call, once per call -> {'known': (B, 6, H, W) fp32 in [0, 1], 'mask': (B, 6 H W) uint8,
        'stays': known_resample - 1, 'score': bool(score_known)}, what the loops take as ``known``"""
        stays = self._check_known()
        device = self.betas.device
        if not torch.is_tensor(known) or tuple(known.shape) != tuple(shape):
            raise ValueError(f'sample_known: known {tuple(known.shape) if torch.is_tensor(known) else type(known).__name__} '
                             f'against the image pair {tuple(shape)}')
        known = known.to(device=device, dtype=torch.float32).contiguous()
        if not bool(((known >= 0.) & (known <= 1.)).all()):  # (a NaN fails both comparisons)
            raise ValueError('sample_known: known has values outside [0, 1], the range of the sampler\'s output and of the '
                             'dataset\'s image channels')
        if isinstance(known_mask, str):
            if known_mask not in self.KNOWN_MASKS:
                raise ValueError(f'sample_known: known_mask = {known_mask!r}: a tensor, or one of {tuple(self.KNOWN_MASKS)}')
            lo, hi = self.KNOWN_MASKS[known_mask]
            kmask = torch.zeros(shape, device=device, dtype=torch.uint8)
            kmask[:, lo:hi] = 1
        else:
            try:
                kmask = (torch.as_tensor(known_mask).to(device) != 0).to(torch.uint8).expand(shape).contiguous()
            except (RuntimeError, TypeError) as e:
                raise ValueError(f'sample_known: known_mask does not broadcast to {tuple(shape)}: {e}') from None
        return {'known': known, 'mask': kmask.reshape(shape[0], -1), 'stays': stays, 'score': bool(self.score_known)}

    @staticmethod
    def _known_state(known, shape, device):
        """the buffers one eager loop keeps: K = 2 * known - 1, the overwritten logits, the score's fp64 workspace"""
        K = ops.affine(known['known'], 2., -1.)
        return {'K': K, 'logits': torch.empty(shape, device=device, dtype=torch.float32), 'ws': ops.known_error_workspace(K)}

    @staticmethod
    def _known_logits(cond, null, computed, cond_scale, known, kst, k, n_entries, tracing):
        """one eager step's logits with the kept elements in them -> (logits, what the trace adds); the update behind it takes
        (logits, None, keep=None).  The score of the entry's own logits first: on the last entry with score_known (it stays in
        ``known['err']``), on every entry when tracing"""
        cs = cond_scale if null is not None else 1.
        more = {}
        if tracing or (known['score'] and k == n_entries - 1):
            err = ops.known_error(cond, null, computed, cs, kst['K'], known['mask'], ws=kst['ws'])
            more['known_err'] = err
            if k == n_entries - 1:
                known['err'] = err
        return ops.known_blend(cond, null, computed, cs, kst['K'], known['mask'], out=kst['logits']), more

    # ---- start from a pair (sample_from; include/dmhomo_hip_start.h has the definition, schedule.start_entry the strength -> entry
    # map).  OPT-IN, through sample_from only: sample() and sample_known() know none of it, every existing result, launch, RNG draw
    # and graph key stays what it is.  The loops take ``start``; their first image is then ca * (2 * init - 1) + cb * eps in ONE launch
    # (dmh_start_mix: eps is the draw sample() uses as its initial image) and they walk the time list from entry k0 on.  Everything
    # per step — every guidance switch, both clip modes, both samplers, known pixels — acts per entry and knows nothing of where the
    # list starts.  What it does to samples of trained weights has not been measured.  The unconditional class does not have it.
    last_start = None                                        # (k0, t*) of the last sample_from call

    def _start_inputs(self, init, strength, shape):
        """the checks of a sample_from call, once per call -> {'init': (B, 6, H, W) fp32 in [0, 1], 'k0': the first entry that
        runs, 't': its time, 'ca', 'cb': the fp32 buffer values q_sample reads at t}, what the loops take as ``start``"""
        k0 = start_entry(self.sampling_timesteps, strength)
        device = self.betas.device
        if not torch.is_tensor(init) or tuple(init.shape) != tuple(shape):
            raise ValueError(f'sample_from: init {tuple(init.shape) if torch.is_tensor(init) else type(init).__name__} '
                             f'against the image pair {tuple(shape)}')
        init = init.to(device=device, dtype=torch.float32).contiguous()
        if not bool(((init >= 0.) & (init <= 1.)).all()):    # (a NaN fails both comparisons)
            raise ValueError('sample_from: init has values outside [0, 1], the range of the sampler\'s output and of the '
                             'dataset\'s image channels')
        host = self._host()
        t = ddim_pairs(self.num_timesteps, self.sampling_timesteps)[k0][0]
        return {'init': init, 'k0': k0, 't': t, 'ca': float(host['sqrt_alphas_cumprod'][t]),
                'cb': float(host['sqrt_one_minus_alphas_cumprod'][t])}

    def _first_image(self, shape, device, start):
        """the image a loop begins with: the generator's first draw of the call, or — ``start`` — the pair noised to its time"""
        if start is None:
            return self.rng.randn(shape, device).contiguous()
        return self.rng.start_mix(start['init'], start['ca'], start['cb'])

    # OPT-IN, None by default (every existing result, launch, RNG draw and graph key stays what it is).  flow_guidance = s_f, a
    # finite number >= 0: classifier-free guidance on the homography condition in sample() — the label of this data set sits in
    # rgb_flow * mask (the class is always 0, DDP:1136), which reaches the network through three stem channels only.  With the switch
    # on the network also runs a "no-flow" pass u (those channels +0.0, null class — at cond_scale == 1: the drawn keep bits) in the
    # same launch sequence (Unet._cond_null_noflow: 3B rows instead of 2B, resp. 2B instead of B), and dmh_flow_guidance_shift
    # moves the logits by e = (s_f - 1) * (n - u) (resp. (s_f - 1) * (c - u)) in front of everything else: the blend behind it is
    # u + s_f * (n - u) + cond_scale * (c - n), the two-scale form of InstructPix2Pix (include/dmhomo_hip.h has the definition).
    # guidance_rescale, apg_eta, photo_guidance, both clip modes, both samplers, every objective, dedup_dropped_rows and the
    # captured step work on the shifted logits unchanged; no random draw is added (flow_guidance = 1. gives the samples of None).
    # Refused with guidance_interval (the gated row lists have no definition for a third pass) and with cfg_mode = 'streams'.
    # model_predictions and forward_with_cond_scale do not know it.  A model learns the no-flow pass only when it is trained with
    # flow_drop_prob > 0 (below): on a model trained without it that pass is out of distribution.  No checkpoint trained with
    # flow_drop_prob exists, and what the switch does to samples of trained weights has not been measured.
    flow_guidance = None

    def _check_flow_guidance(self):
        """-> None (off), or w = flow_guidance - 1 as a float"""
        s = self.flow_guidance
        if s is None:
            return None
        if not (isinstance(s, (int, float)) and not isinstance(s, bool) and 0. <= s < float('inf')):
            raise ValueError(f'flow_guidance = {s!r}: None (off), or a finite number >= 0')
        if self._check_guidance_interval() is not None:
            raise ValueError(f'flow_guidance = {s!r} together with guidance_interval = {self.guidance_interval!r}: the gated row '
                             f'lists have no definition for a third pass')
        if self.model.cfg_mode == 'streams':
            raise ValueError(f"flow_guidance = {s!r} together with cfg_mode = 'streams': the third pass is defined for cfg_mode = "
                             f"'batched' only")
        return float(s) - 1.

    def _flow_network(self, x, t, classes, rgb_flow, mask, cond_scale, w):
        """_network under flow_guidance: the passes with the no-flow one among them, then the shift, in place -> (cond logits,
        null logits or None, computed-rows mask or None) for the code behind _network, unchanged"""
        cond, null, uncond, computed = self.model._cond_null_noflow(x, t, classes, rgb_flow, mask, cond_scale)
        ops.flow_guidance_shift(cond, null, uncond, w, keep=computed)
        return cond, null, computed

    # OPT-IN, 0. by default (nothing is drawn, loss and gradients are bit for bit what they are).  flow_drop_prob = p in [0, 1):
    # training drops the flow condition of a sample with probability p — its normalised rgb_flow is +0.0, the no-flow pass's own
    # input — so that a model learns the pass flow_guidance guides away from.  One (B,) uint8 draw by the route of Unet._keep_mask,
    # directly after the noise draw and before the class-dropout draw; the photometric term keeps flow and mask as they are.
    flow_drop_prob = 0.

    def _check_flow_drop_prob(self):
        p = self.flow_drop_prob
        if not (isinstance(p, (int, float)) and not isinstance(p, bool) and 0. <= p < 1.):
            raise ValueError(f'flow_drop_prob = {p!r}: a number in [0, 1)')
        return float(p)

    def _flow_keep(self, batch, device):
        """the (batch,) uint8 draw of flow_drop_prob (1: the sample keeps its flow condition), or None at 0.: nothing drawn"""
        return self.model._keep_mask(batch, self._check_flow_drop_prob(), device)

    def _pag_network(self, x, t, classes, rgb_flow, mask, cond_scale, s):
        """_network under pag_scale (sampling.py: ScheduleHost.pag_scale): the passes with the perturbed one among them, then
        the shift, in place -> (cond logits, null logits or None, computed-rows mask or None) for the code behind _network,
        unchanged"""
        cond, null, pert, computed = self.model._cond_null_pag(x, t, classes, rgb_flow, mask, cond_scale)
        ops.pag_shift(cond, null, pert, s, keep=computed)
        return cond, null, computed

    def _network(self, x, t, classes, rgb_flow, mask, cond_scale, gate=None):
        """-> (cond logits, null logits or None, computed-rows mask or None): see Unet._cond_null (``gate`` too)"""
        if cond_scale == 1:
            return self.model.forward(x, t, classes, rgb_flow, mask), None, None
        return self.model._cond_null(x, t, classes, rgb_flow, mask, gate)

    def model_predictions(self, x, t, classes, rgb_flow, mask, cond_scale=3., clip_x_start=False):
        """CFG:610-630.  One timestep for the whole batch (what the samplers pass): blend, objective branch and clamp in
        ONE pass of dmh_sampler_step; a timestep per row (p_losses-style callers): the same arithmetic row by row.
        ``clip_x_start=True`` is the static clamp to [-1, 1] whatever ``clip_mode`` says: dynamic thresholding lives in the
        sampling loops only."""
        host = self._host()
        cond, null, computed = self._network(x, t, classes, rgb_flow, mask, cond_scale)
        t0 = self._uniform_time(t)
        if t0 is None:
            if null is not None:                             # null + (cond - null) * cond_scale, CFG:410
                cond, _, _ = ops.sampler_step(self._blend_step(cond_scale), cond, null, null, None, want_x_start=False,
                                              keep=computed)
            return self._predictions_per_row(cond, x.contiguous(), t, clip_x_start)
        step = self._step(host, t0, ops.MODE_LAST, clip_x_start, cond_scale=cond_scale)
        _, x_start, pred_noise = ops.sampler_step(step, cond, null, x.contiguous(), None, True, True, keep=computed)
        return ModelPrediction(pred_noise, x_start)

    def p_mean_variance(self, x, t, classes, cond_scale, clip_denoised=True):
        """CFG:632-637 as it stands: it hands model_predictions ``(x, t, classes, cond_scale)`` — cond_scale in rgb_flow's
        place and no mask — so the call raises TypeError.  Kept failing at the same call."""
        preds = self.model_predictions(x, t, classes, cond_scale)
        x_start = preds.pred_x_start
        if clip_denoised:
            x_start.clamp_(-1., 1.)
        model_mean, posterior_variance, posterior_log_variance = self.q_posterior(x_start=x_start, x_t=x, t=t)
        return model_mean, posterior_variance, posterior_log_variance, x_start

    @torch.no_grad()
    def p_sample(self, x, t: int, classes, cond_scale=3., clip_denoised=True):
        """CFG:639-654: one ancestral step through p_mean_variance — which raises (above), as in the reference."""
        batched_times = torch.full((x.shape[0],), t, device=x.device, dtype=torch.long)
        model_mean, _, model_log_variance, x_start = self.p_mean_variance(x=x, t=batched_times, classes=classes,
                                                                          cond_scale=cond_scale,
                                                                          clip_denoised=clip_denoised)
        b = x.shape[0]
        one = torch.ones((b,), device=x.device, dtype=torch.float32)
        if not t > 0:
            return model_mean, x_start
        noise = self.rng.randn(x.shape, x.device)
        return ops.rows_lincomb(model_mean, one, noise, (0.5 * model_log_variance).exp().reshape(b)), x_start

    @torch.no_grad()
    def ddim_sample(self, classes, rgb_flow, flow, mask, shape, cond_scale=3., clip_denoised=True):
        """CFG:669-711."""
        return self._ddim_sample(classes, rgb_flow, flow, mask, shape, cond_scale, clip_denoised)

    def _ddim_sample(self, classes, rgb_flow, flow, mask, shape, cond_scale=3., clip_denoised=True, trace=None, known=None,
                     start=None):
        """ddim_sample; ``trace`` (list) optionally receives per-step x_start / img for parity tests (and, with clip_mode =
        'dynamic', the step's thresholds 'thr'; with guidance_rescale, its factors 'gfac' at the guided entries; 'guided': whether
        the entry ran with the null pass, False only under guidance_interval; with apg_eta, the step's (A, Cc) per row, 'apg' (B, 2);
        with photo_guidance, the photometric energy of the blend before the correction, 'photo' (B,) float64; with ``known``, the
        score of the entry's logits 'known_err' (B,) float64, and 'stay': True on the stay entries of known_resample).
        known: what _known_inputs returns (sample_known), or None: the loop as it was.  start: what _start_inputs returns
        (sample_from), or None: the loop as it was."""
        batch, device = shape[0], self.betas.device
        steps = self._ddim_steps(clip_denoised, cond_scale, known['stays'] if known else 0, start['k0'] if start else 0)
        guided = self._guided_entries([t for t, _, _ in steps], cond_scale)
        rank = self._dynamic_rank(shape, clip_denoised)
        phi = self._rescale_phi(cond_scale)
        apg = self._apg_on(cond_scale)                       # (refuses guidance_rescale and guidance_interval beside it)
        photo = self._check_photo_guidance()                 # (refuses those two and apg_eta beside it)
        fg = self._check_flow_guidance()                     # None: off, else w.  (It refuses an interval and 'streams'.)
        tag = {} if fg is None else {'flow': True}
        pg = self._check_pag()                               # None: off, else s.  (It refuses flow_guidance, an interval, 'streams'.)
        if pg is not None:
            tag = {'pag': True}
        img = self._first_image(shape, device, start)
        ws = ops.guidance_workspace(img) if phi else None
        ast = self._apg_state(img, apg) if apg else None
        pst = self._photo_state(shape, flow, mask, device) if photo else None
        kst = self._known_state(known, shape, device) if known else None
        for k, (time, step, draws) in enumerate(steps):
            on = guided is None or guided[k]                 # (an unguided entry: the entry at cond_scale == 1, no null pass)
            time_cond = torch.full((batch,), time, device=device, dtype=torch.long)
            if pg is not None:                               # the perturbed pass among the passes, the shift in front of all else
                cond, null, computed = self._pag_network(img, time_cond, classes, rgb_flow, mask, cond_scale, pg)
            elif fg is None:
                cond, null, computed = self._network(img, time_cond, classes, rgb_flow, mask, cond_scale if on else 1)
            else:                                            # the no-flow pass among the passes, and the shift in front of all else
                cond, null, computed = self._flow_network(img, time_cond, classes, rgb_flow, mask, cond_scale, fg)
            noise = self.rng.randn(shape, device).contiguous() if draws else None
            more = {}
            if apg:                                          # the projected logits, then the update without a null pass
                cond, coef = self._apg_logits(step, cond, null, computed, apg, ast)
                null, computed, more = None, None, {'apg': coef}
            if photo:                                        # the corrected logits, then the update without a null pass
                cond, more = self._photo_logits(step, cond, null, computed, photo, pst, cond_scale, trace is not None)
                null, computed = None, None
            if known:                                        # the kept elements over the logits, then the update without a null pass
                cond, kmore = self._known_logits(cond, null, computed, cond_scale, known, kst, k, len(steps), trace is not None)
                null, computed, more = None, None, {**more, **kmore}
            if phi and on:
                img, x_start, extra = self._rescaled_update(step, cond, null, computed, img, noise, None, rank, phi, ws,
                                                            trace is not None)
                if trace is not None:
                    trace.append({'time': time, 'x_start': x_start, 'img': img, 'guided': on, **extra, **tag})
                continue
            if rank is None:
                img, x_start, _ = ops.sampler_step(step, cond, null, img, noise, want_x_start=trace is not None, keep=computed)
                thr = None
            else:
                thr, _ = ops.sampler_threshold(step, cond, null, img, *rank, keep=computed)
                img, x_start = ops.sampler_step_thr(step, cond, null, img, noise, None, thr, want_x_start=trace is not None,
                                                    keep=computed)
            if trace is not None:
                trace.append({'time': time, 'x_start': x_start, 'img': img, 'guided': on, **({} if thr is None else {'thr': thr}),
                              **more, **tag})
                if known and known['stays'] and k % (known['stays'] + 1) != known['stays']:
                    trace[-1]['stay'] = True
        img = ops.affine(img, 0.5, 0.5)                      # unnormalize_to_zero_to_one, CFG:709
        if known:                                            # the kept elements come back as the caller gave them, bit for bit
            ops.known_blend(img, None, None, 1., known['known'], known['mask'])
        return img, mask, flow

    def _dynamic_rank(self, shape, clip):
        """(k, frac) of the row quantile where the loop thresholds dynamically (clip_mode = 'dynamic' and a clipping loop),
        else None: the static clamp, the existing step kernels"""
        if self._check_clip_mode() != 'dynamic' or not clip:
            return None
        return self._quantile_rank(float(self.dynamic_threshold_percentile), shape[1] * shape[2] * shape[3])

    def _rescale_phi(self, cond_scale):
        """phi where the loop rescales its guidance (guidance_rescale > 0 and a null pass to rescale against: cond_scale != 1),
        else 0.: the calls as they were"""
        phi = self._check_guidance_rescale()
        return phi if cond_scale != 1 else 0.

    def _rescaled_update(self, step, cond, null, computed, img, noise, hist, rank, phi, ws, want_x_start):
        """the update of one eager step under guidance_rescale: the factor per row, the threshold of the rescaled blend where
        the loop thresholds dynamically, the step -> (img, x_start or None, what the trace adds)"""
        gfac = ops.guidance_factor(step, cond, null, phi, keep=computed, ws=ws)
        thr = None
        if rank is not None:
            thr, _ = ops.sampler_threshold_gr(step, cond, null, img, gfac, *rank, keep=computed)
        img, x_start = ops.sampler_step_gr(step, cond, null, img, noise, hist, thr, gfac, want_x_start=want_x_start,
                                           keep=computed)
        return img, x_start, {'gfac': gfac, **({} if thr is None else {'thr': thr})}

    def _dpmpp_sample(self, classes, rgb_flow, flow, mask, shape, cond_scale=3., clip_denoised=True, trace=None, known=None,
                      start=None):
        """the loop of _ddim_sample with the multistep solver's update (ScheduleHost._dpmpp_steps; not in the reference): the
        network call — its class-dropout draw included — is the same, the update draws nothing and carries the previous step's
        x_start in ``hist``.  ``trace``, ``known`` and ``start`` as _ddim_sample (no stay entries: _check_known; the solver's
        coefficients are those of the list that begins at start['k0'])."""
        batch, device = shape[0], self.betas.device
        steps = self._dpmpp_steps(clip_denoised, cond_scale, start['k0'] if start else 0)
        guided = self._guided_entries([t for t, _, _ in steps], cond_scale)
        rank = self._dynamic_rank(shape, clip_denoised)
        phi = self._rescale_phi(cond_scale)
        apg = self._apg_on(cond_scale)                       # (refuses guidance_rescale and guidance_interval beside it)
        photo = self._check_photo_guidance()                 # (refuses those two and apg_eta beside it)
        fg = self._check_flow_guidance()                     # None: off, else w.  (It refuses an interval and 'streams'.)
        tag = {} if fg is None else {'flow': True}
        pg = self._check_pag()                               # None: off, else s.  (It refuses flow_guidance, an interval, 'streams'.)
        if pg is not None:
            tag = {'pag': True}
        img = self._first_image(shape, device, start)
        hist = torch.empty_like(img)                         # (entry 0 has c2 == 0: never read before it is written)
        ws = ops.guidance_workspace(img) if phi else None
        ast = self._apg_state(img, apg) if apg else None
        pst = self._photo_state(shape, flow, mask, device) if photo else None
        kst = self._known_state(known, shape, device) if known else None
        for k, (time, step, _) in enumerate(steps):
            on = guided is None or guided[k]                 # (the history carries across guided / unguided entries unchanged)
            time_cond = torch.full((batch,), time, device=device, dtype=torch.long)
            if pg is not None:                               # the perturbed pass among the passes, the shift in front of all else
                cond, null, computed = self._pag_network(img, time_cond, classes, rgb_flow, mask, cond_scale, pg)
            elif fg is None:
                cond, null, computed = self._network(img, time_cond, classes, rgb_flow, mask, cond_scale if on else 1)
            else:                                            # the no-flow pass among the passes, and the shift in front of all else
                cond, null, computed = self._flow_network(img, time_cond, classes, rgb_flow, mask, cond_scale, fg)
            more = {}
            if apg:                                          # the projected logits, then the update without a null pass
                cond, coef = self._apg_logits(step, cond, null, computed, apg, ast)
                null, computed, more = None, None, {'apg': coef}
            if photo:                                        # the corrected logits, then the update without a null pass
                cond, more = self._photo_logits(step, cond, null, computed, photo, pst, cond_scale, trace is not None)
                null, computed = None, None
            if known:                                        # the kept elements over the logits, then the update without a null pass
                cond, kmore = self._known_logits(cond, null, computed, cond_scale, known, kst, k, len(steps), trace is not None)
                null, computed, more = None, None, {**more, **kmore}
            if phi and on:
                img, x_start, extra = self._rescaled_update(step, cond, null, computed, img, None, hist, rank, phi, ws,
                                                            trace is not None)
                if trace is not None:
                    trace.append({'time': time, 'x_start': x_start, 'img': img, 'guided': on, **extra, **tag})
                continue
            if rank is None:
                img, x_start = ops.sampler_step_ms(step, cond, null, img, hist, want_x_start=trace is not None, keep=computed)
                thr = None
            else:
                thr, _ = ops.sampler_threshold(step, cond, null, img, *rank, keep=computed)
                img, x_start = ops.sampler_step_thr(step, cond, null, img, None, hist, thr, want_x_start=trace is not None,
                                                    keep=computed)
            if trace is not None:
                trace.append({'time': time, 'x_start': x_start, 'img': img, 'guided': on, **({} if thr is None else {'thr': thr}),
                              **more, **tag})
                if known and known['stays'] and k % (known['stays'] + 1) != known['stays']:
                    trace[-1]['stay'] = True
        img = ops.affine(img, 0.5, 0.5)                      # unnormalize_to_zero_to_one, CFG:709
        if known:                                            # the kept elements come back as the caller gave them, bit for bit
            ops.known_blend(img, None, None, 1., known['known'], known['mask'])
        return img, mask, flow

    @torch.no_grad()
    def p_sample_loop(self, classes, shape, cond_scale=3.):
        # CFG:656 takes (classes, shape, cond_scale) while CFG:719-720 calls it with six arguments, and
        # CFG:633 mis-passes p_mean_variance's arguments: the reference's ancestral path cannot run
        # (SURVEY.md fact 6).  Kept failing in the same way rather than inventing semantics.
        raise TypeError('classifier_free_guidance.GaussianDiffusion.p_sample_loop is not callable in the reference '
                        '(CFG:656 vs CFG:719-720); use sampling_timesteps < timesteps (DDIM), or the unconditional '
                        'denoising_diffusion_pytorch.GaussianDiffusion for ancestral sampling')

    @torch.no_grad()
    def sample(self, classes, rgb_flow, flow, mask, cond_scale=3.):
        """CFG:713-720."""
        batch_size, image_size, channels = classes.shape[0], self.image_size, self.channels
        shape = (batch_size, channels, image_size, image_size)
        solver = self._check_sampler() == 'dpmpp_2m'         # (walks the time list whatever is_ddim_sampling says)
        if not self.is_ddim_sampling and not solver:
            return self.p_sample_loop(classes, rgb_flow, flow, mask, shape, cond_scale)    # TypeError, as CFG:719-720
        if self.hip_graph and type(self.rng) is DeviceRng and self.sampling_timesteps >= 1:
            return self._sample_graphed(classes, rgb_flow, flow, mask, shape, cond_scale)
        rgb_flow = ops.affine(rgb_flow.to(torch.float32), 2., -1.)      # normalize_to_neg_one_to_one, CFG:716
        if solver:
            return self._dpmpp_sample(classes, rgb_flow, flow, mask, shape, cond_scale)
        return self.ddim_sample(classes, rgb_flow, flow, mask, shape, cond_scale)

    @torch.no_grad()
    def sample_known(self, known, known_mask, classes, rgb_flow, flow, mask, cond_scale=3.):
        """sample() around known pixels (not in the reference; sampling.py: ScheduleHost.known_resample has the description):
        known (B, 6, H, W) fp32 in [0, 1]; known_mask anything that broadcasts to it (nonzero: keep this element), or 'source'
        (channels 0-2) / 'target' (channels 3-5).  -> (img, mask, flow) like sample, the kept elements of img bit for bit those
        of ``known``.  With score_known the call leaves last_known_error (B,) float64."""
        batch_size, image_size, channels = classes.shape[0], self.image_size, self.channels
        shape = (batch_size, channels, image_size, image_size)
        kn = self._known_inputs(known, known_mask, shape)
        solver = self._check_sampler() == 'dpmpp_2m'
        if not self.is_ddim_sampling and not solver:
            return self.p_sample_loop(classes, rgb_flow, flow, mask, shape, cond_scale)    # TypeError, as sample()
        if self.hip_graph and type(self.rng) is DeviceRng and self.sampling_timesteps >= 1:
            out = self._sample_graphed(classes, rgb_flow, flow, mask, shape, cond_scale, known=kn)
        else:
            rgb_flow = ops.affine(rgb_flow.to(torch.float32), 2., -1.)      # normalize_to_neg_one_to_one, CFG:716
            loop = self._dpmpp_sample if solver else self._ddim_sample
            out = loop(classes, rgb_flow, flow, mask, shape, cond_scale, known=kn)
        if kn['score']:
            self.last_known_error = kn['err']
        return out

    @torch.no_grad()
    def sample_from(self, init, strength, classes, rgb_flow, flow, mask, cond_scale=3., known=None, known_mask=None):
        """sample() started from a given pair (SDEdit, Meng et al. 2022 — diffusers' image-to-image ``strength``; not in the
        reference; include/dmhomo_hip_start.h has the definition): init (B, 6, H, W) fp32 in [0, 1] is noised to the time of entry
        k0 = schedule.start_entry(sampling_timesteps, strength) of the time list with the generator's first draw, and the loop runs
        from that entry on: strength * S network entries instead of S.  strength in (0, 1]; 1 runs every entry from q(x_{T-1} |
        init) (pure noise is sample()).  With ``known`` and ``known_mask`` the loop is sample_known's, started from the mixed
        image: the kept elements come back bit for bit, the others start from init.  -> (img, mask, flow) like sample; the call
        leaves last_start = (k0, t*)."""
        batch_size, image_size, channels = classes.shape[0], self.image_size, self.channels
        shape = (batch_size, channels, image_size, image_size)
        if (known is None) != (known_mask is None):
            raise ValueError('sample_from: known and known_mask go together (both, or neither)')
        st = self._start_inputs(init, strength, shape)
        kn = None if known is None else self._known_inputs(known, known_mask, shape)
        solver = self._check_sampler() == 'dpmpp_2m'
        if not self.is_ddim_sampling and not solver:
            return self.p_sample_loop(classes, rgb_flow, flow, mask, shape, cond_scale)    # TypeError, as sample()
        self.last_start = (st['k0'], st['t'])
        if self.hip_graph and type(self.rng) is DeviceRng and self.sampling_timesteps >= 1:
            out = self._sample_graphed(classes, rgb_flow, flow, mask, shape, cond_scale, known=kn, start=st)
        else:
            rgb_flow = ops.affine(rgb_flow.to(torch.float32), 2., -1.)      # normalize_to_neg_one_to_one, CFG:716
            loop = self._dpmpp_sample if solver else self._ddim_sample
            out = loop(classes, rgb_flow, flow, mask, shape, cond_scale, known=kn, start=st)
        if kn is not None and kn['score']:
            self.last_known_error = kn['err']
        return out

    def _graph_tables(self, cond_scale, clip=True, stays=0, first=0):
        """host side of the replayed loop: (steps, times, draws), entry k = the DmhStep, timestep and 'draws noise' flag
        _ddim_sample (or, with sampler = 'dpmpp_2m', _dpmpp_sample) passes at its k-th step (stays: sample_known's stay entries;
        first: the time pairs from ``first`` on, sample_from under 'dpmpp_2m')."""
        times, steps, draws = map(list, zip(*self._sampler_steps(clip, cond_scale, stays, first)))
        return steps, times, draws

    def _sample_graphed(self, classes, rgb_flow, flow, mask, shape, cond_scale, known=None, start=None):
        """sample() with hip_graph (ScheduleHost._replay_captured): one step of CFG:683-707 captured and replayed S times.
        With sampler = 'dpmpp_2m' the step is the network, dmh_sampler_step_ms_dev on a static history buffer and the seek:
        no randn launch is left in it.  With clip_mode = 'dynamic' the update is two calls, dmh_sampler_threshold_dev and
        dmh_sampler_step_thr_dev, on a static scratch and a static threshold per row.  With guidance_rescale (and a null pass)
        the update starts with dmh_guidance_factor_dev on a static factor per row and its static workspace, and the threshold
        and the step are the _gr entries.  With guidance_interval (and a null pass) the same ONE step serves guided and unguided
        entries: a static flag per entry, 'guided', written by fill on every call, is read at the cursor by dmh_rows_gated (the row
        lists of the network: no null rows at an unguided entry) and by dmh_guidance_gate behind the network (null <- cond there),
        and every launch behind the gate is the one it was.  With apg_eta (and a null pass) the update starts with dmh_apg_coef_dev and
        dmh_apg_apply on static buffers (the guided logits, the coefficients, the fp64 workspace and, with momentum, the running
        average, which fill zeroes on every call), and the launches behind them are those of cond_scale == 1 on the guided logits.
        With photo_guidance the update starts with dmh_photo_guide_dev on static buffers (flow and mask as fp32, the preconditioner
        s, the fixed-point accumulator, the guided logits): fill copies flow and mask and recomputes s on every call, the weight
        is a launch argument and so part of the key.  With flow_guidance the network is Unet._cond_null_noflow and
        dmh_flow_guidance_shift stands in front of the update: no static buffer more, w = flow_guidance - 1 is a launch argument and
        so part of the key.  With pag_scale the network is Unet._cond_null_pag and dmh_pag_shift stands in front of the update
        in the same way: s = pag_scale is a launch argument and so part of the key.  With ``known`` (sample_known) dmh_known_blend stands
        between those and the update on static buffers (K, known, the expanded mask, the overwritten logits; with score_known the
        fp64 workspace and the result, written by dmh_known_error in the last step only): fill copies this call's known and mask,
        whose values are not part of the key — only that the feature is on, known_resample and score_known are —, the stay entries
        are entries of the step table, and last() ends with the unnormalise and the write-back.  With ``start`` (sample_from) fill writes
        st['img'] with dmh_start_mix instead of the first draw and the replay begins at a later entry.  Under 'ddim' the table is the full
        table and nothing about the start is in the key: the call replays sample()'s (or sample_known's) capture from entry k0 *
        (stays + 1) on, and changing strength or init never captures again.  Under 'dpmpp_2m' the coefficients depend on k0: the table is
        built over pairs[k0:] and the key gains ('first', k0), only when k0 > 0."""
        m, eng, device = self.model, self.model._engine, classes.device
        clip = True                                          # ddim_sample's clip_denoised default, as sample() calls it
        solver = self._check_sampler() == 'dpmpp_2m'
        rank = self._dynamic_rank(shape, clip)               # None: the static clamp
        phi = self._rescale_phi(cond_scale)                  # 0.: no rescale
        gated = self._check_guidance_interval() is not None and cond_scale != 1      # (the interval's VALUE is not baked in)
        apg = self._apg_on(cond_scale)                       # None: off.  (It refuses phi and an interval beside it.)
        # everything besides weights, schedule and device that is baked into the captured launches or the step tables
        key = (tuple(shape), tuple(rgb_flow.shape), float(cond_scale), m.cfg_mode, int(m.stream_splits),
               bool(m.dedup_dropped_rows), float(m.cond_drop_prob), self.sampling_timesteps,
               self.num_timesteps, self.objective, float(self.ddim_sampling_eta), clip, self.rng.graph_key(), self.sampler,
               self.clip_mode, None if rank is None else float(self.dynamic_threshold_percentile),
               float(self.guidance_rescale))
        if gated:
            key = key + ('guidance_interval',)
        if apg:
            key = key + (('apg',) + apg,)
        photo = self._check_photo_guidance()                 # None: off.  (It refuses phi, apg_eta and an interval beside it.)
        if photo:
            key = key + (('photo', photo),)
        fg = self._check_flow_guidance()                     # None: off, else w.  (It refuses an interval and 'streams'.)
        if fg is not None:                                   # (w is a launch argument of the shift: baked into the capture)
            key = key + (('flow_guidance', fg),)
        pg = self._check_pag()                               # None: off, else s.  (It refuses flow_guidance, an interval, 'streams'.)
        if pg is not None:                                   # (s is a launch argument of the shift: baked into the capture)
            key = key + (('pag_scale', pg),)
        stays = known['stays'] if known else 0
        if known:                                            # (the table's length and the score's launches: baked in; the pixels not)
            key = key + (('known', stays + 1, known['score']),)
        k0 = start['k0'] if start else 0
        tfirst = k0 if solver else 0                         # the pair the capture's table begins at
        if tfirst:                                           # (the solver's coefficients over pairs[k0:]: baked into the table)
            key = key + (('first', k0),)

        def buffers(st, times, draws):
            ins = st['ins'] = [classes.clone(), rgb_flow.to(torch.float32).clone(), mask.clone()]
            st['rf'] = torch.empty_like(ins[1])
            ops.affine(ins[1], 2., -1., out=st['rf'])        # (the warm-up's input)
            # the embedding side of the network depends on (step, class, keep bit) only: tables, made once per capture
            T_tab, C_tab = eng.ss_tables(times)
            st['ss_tab'] = (T_tab, C_tab, st['cursor'])

            if solver:
                st['hist'] = torch.zeros(shape, device=device)
            if rank is not None:                             # dynamic thresholding: scratch for the raw x_start, a threshold per row
                st['x0_raw'] = torch.zeros(shape, device=device)
                st['thr'] = torch.ones((shape[0],), device=device)
            if phi:                                          # guidance rescale: a factor per row, the fp64 partial moments
                st['gfac'] = torch.ones((shape[0],), device=device)
                st['gws'] = ops.guidance_workspace(st['img'])
            if gated:                                        # guidance interval: a flag per entry (all guided until fill writes it)
                st['guided'] = torch.ones((len(times),), device=device, dtype=torch.uint8)
            if apg:                                          # adaptive projected guidance: the guided logits, (A, Cc) per row,
                st['apg_guided'] = torch.zeros(shape, device=device)         # the fp64 partial sums, the running average
                st['apg_coef'] = torch.ones((shape[0], 2), device=device)
                st['apg_ws'] = ops.apg_workspace(st['img'])
                st['apg_run'] = torch.zeros(shape, device=device) if apg[2] != 0. else None
            if photo:                                        # photometric guidance: flow and mask as fp32, s, the accumulator
                st['photo_flow'] = flow.to(torch.float32).clone()            # (zero between launches), the guided logits
                st['photo_mask'] = mask.to(torch.float32).clone()
                st['photo_acc'] = ops.photo_acc(shape[0], shape[2], shape[3], device)
                st['photo_s'] = ops.photo_weights(st['photo_flow'], st['photo_mask'], st['photo_acc'])
                st['photo_guided'] = torch.zeros(shape, device=device)
            if known:                                        # known pixels: K, known, the mask (nothing kept until fill writes it),
                st['known_K'] = torch.zeros(shape, device=device)            # the overwritten logits, the score's buffers
                st['known_01'] = torch.zeros(shape, device=device)
                st['known_mask'] = torch.zeros((shape[0], shape[1] * shape[2] * shape[3]), device=device, dtype=torch.uint8)
                st['known_logits'] = torch.zeros(shape, device=device)
                if known['score']:
                    st['known_ws'] = ops.known_error_workspace(st['img'])
                    st['known_err'] = torch.zeros((shape[0],), device=device, dtype=torch.float64)
            gate = (st['cursor'], st['guided']) if gated else None

            def network():                                   # -> the logits the update reads
                if pg is not None:                           # the perturbed pass among the passes, the shift in front of all else
                    return self._pag_network(st['img'], st['tcond'], ins[0], st['rf'], ins[2], cond_scale, pg)
                if fg is not None:                           # the no-flow pass among the passes, the shift in front of all else
                    return self._flow_network(st['img'], st['tcond'], ins[0], st['rf'], ins[2], cond_scale, fg)
                if gate is None:
                    return self._network(st['img'], st['tcond'], ins[0], st['rf'], ins[2], cond_scale)
                cond, null, computed = self._network(st['img'], st['tcond'], ins[0], st['rf'], ins[2], cond_scale, gate)
                ops.guidance_gate(*gate, cond, null)         # an unguided entry: null <- cond, the update below is the unguided one
                return cond, null, computed

            def step(cond, null, computed, noise, out, final=False):     # the update of the entry at the cursor
                hist = st['hist'] if solver else None
                if apg:                                      # the projected logits, then the update without a null pass
                    ops.apg_coef_dev(st['cur'], cond, null, *apg, keep=computed, run=st['apg_run'], ws=st['apg_ws'],
                                     coef=st['apg_coef'])
                    cond = ops.apg_apply(cond, null, st['apg_coef'], keep=computed, run=st['apg_run'], out=st['apg_guided'])
                    null = computed = None
                if photo:                                    # the corrected logits, then the update without a null pass
                    cond = ops.photo_guide_dev(st['cur'], cond, null, computed, st['photo_flow'], st['photo_mask'], st['photo_s'],
                                               photo, st['photo_acc'], out=st['photo_guided'])
                    null = computed = None
                if known:                                    # the kept elements over the logits, then the update without a null pass
                    cs = cond_scale if null is not None else 1.
                    if final and known['score']:             # the score of the last entry's own logits
                        ops.known_error(cond, null, computed, cs, st['known_K'], st['known_mask'], ws=st['known_ws'],
                                        out=st['known_err'])
                    cond = ops.known_blend(cond, null, computed, cs, st['known_K'], st['known_mask'], out=st['known_logits'])
                    null = computed = None
                if phi:
                    ops.guidance_factor_dev(st['cur'], cond, null, phi, keep=computed, ws=st['gws'], gfac=st['gfac'])
                    if rank is not None:
                        ops.sampler_threshold_gr_dev(st['cur'], cond, null, st['img'], st['gfac'], *rank, keep=computed,
                                                     x0_raw=st['x0_raw'], thr=st['thr'])
                    return ops.sampler_step_gr_dev(st['cur'], cond, null, st['img'], noise, hist,
                                                   None if rank is None else st['thr'], st['gfac'], out=out, keep=computed)
                if rank is not None:
                    ops.sampler_threshold_dev(st['cur'], cond, null, st['img'], *rank, keep=computed, x0_raw=st['x0_raw'],
                                              thr=st['thr'])
                    return ops.sampler_step_thr_dev(st['cur'], cond, null, st['img'], noise, hist, st['thr'], out=out,
                                                    keep=computed)
                if solver:
                    return ops.sampler_step_ms_dev(st['cur'], cond, null, st['img'], hist, out=out, keep=computed)
                return ops.sampler_step_dev(st['cur'], cond, null, st['img'], noise, out=out, keep=computed)

            def mid():                                       # one denoise step of CFG:684-707, in place on st['img']
                logits = network()
                step(*logits, None if solver else self.rng.randn(shape, device).contiguous(), st['img'])
                ops.sampler_seek(st['cursor'], -1, st['table'], st['times'], st['cur'], st['tcond'])

            def last():                                      # CFG:693-695 + unnormalize, CFG:709
                logits = network()
                out = ops.affine(step(*logits, None, None, final=True), 0.5, 0.5)
                if known:                                    # the kept elements come back as the caller gave them, bit for bit
                    ops.known_blend(out, None, None, 1., st['known_01'], st['known_mask'])
                return out
            return mid, last

        def fill(st):
            for dst, src in zip(st['ins'], (classes, rgb_flow, mask)):
                dst.copy_(src)
            ops.affine(st['ins'][1], 2., -1., out=st['rf'])  # normalize_to_neg_one_to_one, CFG:716
            if start is None:
                st['img'].copy_(self.rng.randn(shape, device))   # CFG:679
            else:                                            # the pair noised to the time of entry k0, with that same draw
                self.rng.start_mix(start['init'], start['ca'], start['cb'], out=st['img'])
            if apg and st['apg_run'] is not None:
                st['apg_run'].zero_()                        # the running average starts every loop at zero
            if photo:                                        # this call's flow and mask, and the preconditioner they give
                st['photo_flow'].copy_(flow)
                st['photo_mask'].copy_(mask)
                ops.photo_weights(st['photo_flow'], st['photo_mask'], st['photo_acc'], out=st['photo_s'])
            if known:                                        # this call's pixels and mask
                st['known_01'].copy_(known['known'])
                ops.affine(st['known_01'], 2., -1., out=st['known_K'])
                st['known_mask'].copy_(known['mask'])
            if gated:
                flags = self._guided_entries(self._graph_tables(cond_scale, clip, stays, tfirst)[1], cond_scale)
                st['guided'].copy_(torch.tensor(flags, dtype=torch.uint8))
        first = (k0 - tfirst) * (stays + 1)                  # the entry of the capture's table the replay begins at
        img = self._replay_captured(shape, device, key, lambda: self._graph_tables(cond_scale, clip, stays, tfirst), buffers, fill,
                                    **({'first': first} if first else {}))
        if known and known['score']:
            known['err'] = self.__dict__['_graph_state']['known_err'].clone()
        return img, mask, flow

    @torch.no_grad()
    def interpolate(self, x1, x2, t=None, lam=0.5):
        """CFG:722-736 calls ``self.p_sample(img, t)`` — two arguments for a method that needs classes and conditions
        (CFG:639-654), and p_sample itself mis-calls p_mean_variance: it raises TypeError in the
        reference for any t > 0, and so does this."""
        raise TypeError('classifier_free_guidance.GaussianDiffusion.interpolate is not callable in the reference '
                        '(CFG:733 vs CFG:639); use denoising_diffusion_pytorch.GaussianDiffusion.interpolate')

    @torch.no_grad()
    def p_losses(self, x_start, t, *, classes, rgb_flow, flow, mask, noise=None):
        """CFG:770-806, the loss VALUE: q_sample -> UNet (class dropout p=0.5) -> flow_warp -> L1/L2 + alpha_bar_t-weighted
        masked photometric term.  No autograd graph is built here; ``forward`` returns a loss with a grad_fn whose
        gradients come from the HIP backward kernels of dmhomo_amd.train (same forward, activations saved)."""
        from .ddpm import flow_warp
        squared = self.loss_fn == 'l2'
        noise = default(noise, lambda: self.rng.randn(x_start.shape, x_start.device))
        x_start = x_start.to(torch.float32).contiguous()
        noise = noise.to(torch.float32).contiguous()
        t = t.to(torch.int64).contiguous()
        x = self.q_sample(x_start, t, noise)
        flow_keep = self._flow_keep(x_start.shape[0], x_start.device)    # flow_drop_prob: drawn behind the noise, before the class
        if flow_keep is not None:                            # dropout.  (rgb_flow arrives normalised: 1 * v + 0 on kept rows)
            rgb_flow = ops.affine_rows_keep(rgb_flow.to(torch.float32), 1., 0., flow_keep)
        model_out = self.model(x, t, classes, rgb_flow=rgb_flow, mask=mask)
        im1, im2 = model_out[:, :3].contiguous(), model_out[:, 3:].contiguous()
        im2_warp = flow_warp(im2, flow)
        target = self._loss_target(x_start, t, noise)
        loss = ops.diff_mean(model_out, target, None, squared)
        photo = ops.diff_mean(im2_warp, im1, mask.to(torch.float32).contiguous(), squared)
        w = self.alphas_cumprod.gather(-1, t).contiguous()
        return ops.loss_combine(loss, photo, w)

    def forward(self, img, *args, **kwargs):
        """CFG:808-842: split the 12-channel batch (DDP:1162 layout), draw t, evaluate p_losses.

        With autograd enabled and trainable parameters the returned loss carries a grad_fn: ``loss.backward()`` fills
        ``parameter.grad`` exactly as the reference's does, so a user-written loop (``loss = diffusion(batch,
        classes=c); loss.backward(); opt.step()``, DDP:1843-1857) runs unchanged — the gradients come from the HIP
        backward kernels of dmhomo_amd.train (no autograd graph inside), computed together with the loss.  Under
        ``torch.no_grad()`` only the value is evaluated."""
        classes = kwargs.get('classes', args[0] if args else None)
        if torch.is_grad_enabled() and classes is not None and any(p.requires_grad for p in self.model.parameters()):
            from .train import loss_with_grad_fn
            return loss_with_grad_fn(self, img, classes)
        b, c, h, w = img.shape
        assert h == self.image_size and w == self.image_size, f'height and width of image must be {self.image_size}'
        t = torch.randint(0, self.num_timesteps, (b,), device=img.device).long()
        data = ops.affine(img[:, :6].to(torch.float32), 2., -1.)
        mask = img[:, 6:7].contiguous()
        rgb_flow = ops.affine(img[:, -5:-2].to(torch.float32), 2., -1.)
        flow = img[:, -2:].contiguous()
        return self.p_losses(data, t, *args, rgb_flow=rgb_flow, flow=flow, mask=mask, **kwargs)
