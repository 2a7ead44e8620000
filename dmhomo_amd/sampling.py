"""What the conditional (``cfg``) and the unconditional (``ddpm``) GaussianDiffusion share on the sampling side: the
reference's small helpers, the device noise source, the host mirrors of the schedule with the per-step ``DmhStep``
records built from them, and the captured-and-replayed sampling loop (``hip_graph``)."""
from collections import OrderedDict, namedtuple
import math

import torch

from . import ops
from ._lib import DmhStep, graph_capture
from .schedule import ddim_pairs, make_buffers

ModelPrediction = namedtuple('ModelPrediction', ['pred_noise', 'pred_x_start'])


def exists(x):
    return x is not None


def default(val, d):
    if exists(val):
        return val
    return d() if callable(d) else d


def extract(a, t, x_shape):
    """D3, CFG:472-475: a.gather(-1, t) shaped (b, 1, ..., 1) (integer indexing: tensor plumbing)."""
    b, *_ = t.shape
    out = a.gather(-1, t)
    return out.reshape(b, *((1,) * (len(x_shape) - 1)))


class DeviceRng:
    """The noise source of the samplers, drawn in the reference's call order (CFG:679 randn(shape), CFG:90
    zeros(B).uniform_(0,1), CFG:703 randn_like).

    Default: torch's generator of the target device — the reference's own behaviour: row b of a draw depends on how many
    rows the process holds and on the process's seed.
    After ``key_by_sample(seed, sample_ids)``: every value is a pure function of (seed, GLOBAL sample id, draw index,
    element) (``dmh_rng_indexed``: Philox4x32-10 + Box-Muller; the draw index lives in device memory and advances with
    every launch, also inside a replayed HIP graph) — a batch sharded over N ranks, each keyed with its own slice of the
    sample ids, reproduces the single-GPU batch row for row, bit for bit."""

    def __init__(self):
        self.sample_ids = None           # (B,) int64 device tensor once keyed
        self.state = None                # (4,) int64 device tensor: seed, draw index, tickets, reserved

    def key_by_sample(self, seed, sample_ids, device=None):
        """sample_ids: the GLOBAL indices of this process's rows (``range(lo, hi)`` of distributed.shard_bounds), in row
        order.  Re-keying with the same number of rows on the same device keeps the tensors' storage (a captured graph
        stays valid) and restarts the draw index at 0."""
        ids = torch.as_tensor(list(sample_ids), dtype=torch.int64)
        device = torch.device(device) if device is not None else (self.sample_ids.device if self.sample_ids is not None
                                                                 else torch.device('cuda', torch.cuda.current_device()))
        state = torch.tensor([int(seed), 0, 0, 0], dtype=torch.int64)
        if self.sample_ids is not None and self.sample_ids.shape == ids.shape and self.sample_ids.device == device:
            self.sample_ids.copy_(ids)
            self.state.copy_(state)
        else:
            self.sample_ids, self.state = ids.to(device), state.to(device)
        return self

    def unkey(self):
        self.sample_ids = self.state = None
        return self

    @property
    def keyed(self):
        return self.sample_ids is not None

    def graph_key(self):
        """what a captured launch of this generator bakes in"""
        return None if not self.keyed else (self.sample_ids.data_ptr(), self.state.data_ptr(), int(self.sample_ids.shape[0]))

    def snapshot(self, device):
        """state to put back with ``restore`` (the eager warm-up in front of a graph capture must not consume draws)"""
        if self.keyed:
            return ('indexed', self.state.clone())
        return ('stream', torch.cuda.get_rng_state(device))

    def restore(self, snap, device):
        if snap[0] == 'indexed':
            self.state.copy_(snap[1])
        else:
            torch.cuda.set_rng_state(snap[1], device)

    def ids_for(self, n):
        """the sample ids of a draw with n rows: all of them, or — a short last batch of a loader that keeps it, as the
        reference's DataLoader does (DDP:1746-1752) — the first n (a view: same storage, so a captured graph keyed on the
        full-size batch is not disturbed)"""
        n = int(n)
        if n > self.sample_ids.shape[0]:
            raise ValueError(f'the generator is keyed for {self.sample_ids.shape[0]} rows, a draw asks for {n}: '
                             f'key_by_sample with the ids of this batch first')
        return self.sample_ids if n == self.sample_ids.shape[0] else self.sample_ids[:n]

    def randn(self, shape, device):
        if self.keyed:
            return ops.rng_indexed(shape, self.ids_for(shape[0]), self.state, 0)
        return torch.randn(tuple(shape), device=device)

    def uniform(self, n, device):
        if self.keyed:
            return ops.rng_indexed((n,), self.ids_for(n), self.state, 1)
        return torch.zeros((n,), device=device).float().uniform_(0, 1)

    def start_mix(self, init01, ca, cb, out=None):
        """ca * (2 * init01 - 1) + cb * eps with eps the next randn(init01.shape) of this generator, in one launch of
        dmh_start_mix: keyed, the kernel draws eps itself and advances the draw index; else torch's generator draws it and the
        kernel reads it.  -> out"""
        if self.keyed:
            return ops.start_mix(init01, ca, cb, sample_ids=self.ids_for(init01.shape[0]), state=self.state, out=out)
        noise = self.randn(init01.shape, init01.device)
        return ops.start_mix(init01, ca, cb, noise=noise, out=noise if out is None else out)


class ScheduleHost:
    """what the two GaussianDiffusion classes share.  The constructor body, q_sample, the loss target.  Host mirrors of the
    schedule buffers: the reference indexes device buffers with python ints and does 0-dim fp32 tensor arithmetic on them
    (CFG:697-701); here the same ops run on CPU copies and the results enter the sampler kernel as scalars (``DmhStep``).
    And the replayed sampling loop."""

    def _init_diffusion(self, model, image_size, timesteps, sampling_timesteps, loss_type, objective, beta_schedule,
                        p2_loss_weight_gamma, p2_loss_weight_k, ddim_sampling_eta):
        """the body of GaussianDiffusion.__init__, CFG:500-584 [DDP:483-582]; buffers and their names as the reference"""
        # (``type(self) == GaussianDiffusion`` in the reference: the two classes are the direct subclasses of this one)
        assert not (ScheduleHost in type(self).__bases__ and model.channels != model.out_dim)
        assert not model.random_or_learned_sinusoidal_cond
        self.model = model
        self.channels = self.model.channels
        self.image_size = image_size
        self.objective = objective
        assert objective in {'pred_noise', 'pred_x0', 'pred_v'}, \
            'objective must be either pred_noise (predict noise) or pred_x0 (predict image start) or pred_v (predict v)'
        bufs = make_buffers(beta_schedule, timesteps, p2_loss_weight_gamma, p2_loss_weight_k)
        self.num_timesteps = int(bufs['betas'].shape[0])
        self.loss_type = loss_type
        self.sampling_timesteps = default(sampling_timesteps, timesteps)
        assert self.sampling_timesteps <= timesteps
        self.is_ddim_sampling = self.sampling_timesteps < timesteps
        self.ddim_sampling_eta = ddim_sampling_eta
        for name, val in bufs.items():
            self.register_buffer(name, val)

    def q_sample(self, x_start, t, noise=None):
        """CFG:738-742 [DDP:756-761]."""
        noise = default(noise, lambda: self.rng.randn(x_start.shape, x_start.device))
        ca = self.sqrt_alphas_cumprod.gather(-1, t).contiguous()
        cb = self.sqrt_one_minus_alphas_cumprod.gather(-1, t).contiguous()
        return ops.q_sample(x_start.contiguous(), noise.contiguous(), ca, cb)

    @property
    def loss_fn(self):
        """CFG:744-751 [DDP:763-770] — the name of the elementwise loss (the reduction runs in dmh_diff_mean)."""
        if self.loss_type in ('l1', 'l2'):
            return self.loss_type
        raise ValueError(f'invalid loss type {self.loss_type}')

    def _pred_x_start(self, x, t, model_out):
        """model_predictions(x, t, ...).pred_x_start for a given UNet output (DDP:582-600, no clamp): per-sample
        coefficients, t differs from row to row"""
        if self.objective == 'pred_x0':
            return model_out
        ca = (self.sqrt_recip_alphas_cumprod if self.objective == 'pred_noise' else self.sqrt_alphas_cumprod)
        cb = (self.sqrt_recipm1_alphas_cumprod if self.objective == 'pred_noise' else self.sqrt_one_minus_alphas_cumprod)
        return ops.q_sample(x, model_out.contiguous(), ca.gather(-1, t).contiguous(), (-cb).gather(-1, t).contiguous())

    def _loss_target(self, x_start, t, noise):
        """what the UNet output is compared with (CFG:786-794 [DDP:795-803]): the one statement of it, for the loss value
        of both classes and both training steps"""
        if self.objective == 'pred_noise':
            return noise
        if self.objective == 'pred_x0':
            return x_start
        if self.objective == 'pred_v':                       # predict_v, CFG:596-598
            return ops.q_sample(noise, x_start, self.sqrt_alphas_cumprod.gather(-1, t).contiguous(),
                                (-self.sqrt_one_minus_alphas_cumprod).gather(-1, t).contiguous())
        raise ValueError(f'unknown objective {self.objective}')

    _HOST_NAMES = ('alphas_cumprod', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'sqrt_alphas_cumprod',
                   'sqrt_one_minus_alphas_cumprod', 'posterior_mean_coef1', 'posterior_mean_coef2',
                   'posterior_log_variance_clipped')

    def _host(self):
        """CPU copies of the schedule buffers, cached per buffer version (a device -> host copy per sampling call would
        also be illegal inside a HIP-graph capture)."""
        sig = tuple((getattr(self, n).data_ptr(), getattr(self, n)._version) for n in self._HOST_NAMES)
        cache = self.__dict__.get('_host_cache')
        if cache is None or cache[0] != sig:
            cache = (sig, {n: getattr(self, n).detach().cpu() for n in self._HOST_NAMES})
            self.__dict__['_host_cache'] = cache
        return cache[1]

    # ---- D4 / D7: the affine combinations of CFG:586-608 [DDP:584-611] with a timestep per row
    def _at(self, name, t, neg=False):
        a = getattr(self, name)
        return (-a if neg else a).gather(-1, t.to(torch.int64)).contiguous()

    def predict_start_from_noise(self, x_t, t, noise):
        """CFG:586-588: extract(sqrt_recip_ac) * x_t - extract(sqrt_recipm1_ac) * noise."""
        return ops.rows_lincomb(x_t, self._at('sqrt_recip_alphas_cumprod', t), noise,
                                self._at('sqrt_recipm1_alphas_cumprod', t, neg=True))

    def predict_noise_from_start(self, x_t, t, x0):
        """CFG:590-594: (extract(sqrt_recip_ac) * x_t - x0) / extract(sqrt_recipm1_ac)."""
        minus_one = torch.full((x_t.shape[0],), -1., device=x_t.device, dtype=torch.float32)
        return ops.rows_lincomb(x_t, self._at('sqrt_recip_alphas_cumprod', t), x0, minus_one,
                                div=self._at('sqrt_recipm1_alphas_cumprod', t))

    def predict_v(self, x_start, t, noise):
        """CFG:596-598: extract(sqrt_ac) * noise - extract(sqrt_1m_ac) * x_start."""
        return ops.rows_lincomb(noise, self._at('sqrt_alphas_cumprod', t), x_start,
                                self._at('sqrt_one_minus_alphas_cumprod', t, neg=True))

    def predict_start_from_v(self, x_t, t, v):
        """CFG:600-601: extract(sqrt_ac) * x_t - extract(sqrt_1m_ac) * v."""
        return ops.rows_lincomb(x_t, self._at('sqrt_alphas_cumprod', t), v,
                                self._at('sqrt_one_minus_alphas_cumprod', t, neg=True))

    def q_posterior(self, x_start, x_t, t):
        """CFG:603-608: (posterior mean, variance, clipped log variance), the last two shaped (b, 1, 1, 1)."""
        mean = ops.rows_lincomb(x_start, self._at('posterior_mean_coef1', t), x_t, self._at('posterior_mean_coef2', t))
        return (mean, extract(self.posterior_variance, t, x_t.shape),
                extract(self.posterior_log_variance_clipped, t, x_t.shape))

    def _predictions_per_row(self, model_output, x, t, clip_x_start):
        """the objective branch of model_predictions (CFG:614-628) for a batch whose rows sit at different timesteps"""
        one = torch.ones((x.shape[0],), device=x.device, dtype=torch.float32)
        clip = (lambda v: ops.rows_lincomb(v, one, clamp=True)) if clip_x_start else (lambda v: v)
        if self.objective == 'pred_noise':
            pred_noise = model_output
            x_start = clip(self.predict_start_from_noise(x, t, pred_noise))
        elif self.objective == 'pred_x0':
            x_start = clip(model_output)
            pred_noise = self.predict_noise_from_start(x, t, x_start)
        else:                                                # pred_v
            x_start = clip(self.predict_start_from_v(x, t, model_output))
            pred_noise = self.predict_noise_from_start(x, t, x_start)
        return ModelPrediction(pred_noise, x_start)

    @staticmethod
    def _uniform_time(t):
        """python int when every row shares the timestep (always true while sampling), else None"""
        t0 = int(t[0])
        if t.numel() > 1 and not bool((t == t0).all()):
            return None
        return t0

    # ---- the per-step records of dmh_sampler_step (one fused pass: guidance blend, objective branch, clamp, update)
    def _step(self, host, t, mode, clip, c=(0., 0., 0.), cond_scale=1.):
        return DmhStep(objective=ops.OBJECTIVE[self.objective], clip=int(bool(clip)), mode=mode,
                       cond_scale=float(cond_scale),
                       sqrt_recip_ac=float(host['sqrt_recip_alphas_cumprod'][t]),
                       sqrt_recipm1_ac=float(host['sqrt_recipm1_alphas_cumprod'][t]),
                       sqrt_ac=float(host['sqrt_alphas_cumprod'][t]),
                       sqrt_1m_ac=float(host['sqrt_one_minus_alphas_cumprod'][t]),
                       c0=float(c[0]), c1=float(c[1]), c2=float(c[2]))

    @staticmethod
    def _blend_step(cond_scale):
        """the guidance blend alone, null + (cond - null) * cond_scale (CFG:410), as a step: the logits pass through as x0"""
        return DmhStep(objective=ops.OBJECTIVE['pred_x0'], clip=0, mode=ops.MODE_LAST, cond_scale=float(cond_scale),
                       sqrt_recip_ac=1., sqrt_recipm1_ac=1.)

    def _ddim_coef(self, host, time, time_next):
        """sqrt(alpha_next), c, sigma in the reference's op order, CFG:697-701."""
        alpha = host['alphas_cumprod'][time]
        alpha_next = host['alphas_cumprod'][time_next]
        sigma = self.ddim_sampling_eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
        # For a first jump from t=T-1 (alpha ~ 2e-9) to alpha_next >~ 1e-2 (s_step <= 8) the radicand is pure fp32
        # cancellation noise of +-6e-8 and the reference yields c = NaN on hosts whose sqrt rounds the other way
        # (seen: 999 -> 499).  Clamping at 0 changes nothing where the reference is finite.
        c = (1 - alpha_next - sigma ** 2).clamp(min=0).sqrt()
        return float(alpha_next.sqrt()), float(c), float(sigma)

    def _stay_coef(self, host, time, time_next):
        """(c0, c1, c2) of a "stay" entry time -> time in front of the entry time -> time_next (known_resample): the entry's
        DDIM step followed by re-noising back to ``time`` is, in distribution, one DDIM update with a = abar[time], a' =
        abar[time_next] (1 for the entry that returns x_0) and that entry's (sigma, c) (0, 0 for the last):  c0 = sqrt(a), c1 =
        sqrt(a / a') c, c2 = sqrt((a / a') sigma^2 + 1 - a / a'), so that c1^2 + c2^2 = 1 - a.  float64 from the fp32
        alphas_cumprod buffer, sigma and c by the formulas of _ddim_coef."""
        abar = host['alphas_cumprod'].double()
        a = float(abar[time])
        if time_next < 0:
            a1, sigma, c = 1., 0., 0.
        else:
            a1 = float(abar[time_next])
            sigma = float(self.ddim_sampling_eta) * math.sqrt((1. - a / a1) * (1. - a1) / (1. - a))
            c = math.sqrt(max(1. - a1 - sigma * sigma, 0.))
        q = a / a1
        return math.sqrt(a), math.sqrt(q) * c, math.sqrt(q * sigma * sigma + 1. - q)

    def _ddim_steps(self, clip, cond_scale=1., stays=0, first=0):
        """the DDIM loop (CFG:683-707, DDP:700-726) as a list of (time, DmhStep, draws noise): every step but the last
        draws noise and moves to time_next; the last (time_next < 0) returns x_start and draws nothing.  The eager loops
        and the replayed loop's step tables all read this list.  stays (known_resample - 1, sample_known only): that many
        "stay" entries time -> time in front of every entry (_stay_coef), each a DDIM update that draws noise.  first (sample_from:
        schedule.start_entry): the list over the time pairs from ``first`` on — the tail of the full list, each pair's stays with it."""
        host = self._host()
        steps = []
        for time, time_next in ddim_pairs(self.num_timesteps, self.sampling_timesteps)[first:]:
            for _ in range(stays):
                steps.append((time, self._step(host, time, ops.MODE_DDIM, clip, self._stay_coef(host, time, time_next),
                                               cond_scale), 1))
            if time_next < 0:
                steps.append((time, self._step(host, time, ops.MODE_LAST, clip, cond_scale=cond_scale), 0))
            else:
                steps.append((time, self._step(host, time, ops.MODE_DDIM, clip, self._ddim_coef(host, time, time_next),
                                               cond_scale), 1))
        return steps

    # OPT-IN, 'ddim' by default (every existing result stays what it is).  'dpmpp_2m': sample() of both classes runs the
    # second-order multistep solver DPM-Solver++ 2M in data prediction (Lu et al. 2022; the reference has no such solver) over
    # the same ``sampling_timesteps`` time list as DDIM, whatever is_ddim_sampling says.  Deterministic: no per-step noise, and
    # ``ddim_sampling_eta`` is ignored.  On an analytic Gaussian model its discretisation error at 16 steps is below DDIM's
    # (eta = 0) at 32 (tests/test_solver_host.py); what it does to samples of trained weights has not been measured.
    sampler = 'ddim'
    SAMPLERS = ('ddim', 'dpmpp_2m')

    def _check_sampler(self):
        if self.sampler not in self.SAMPLERS:
            raise ValueError(f'unknown sampler {self.sampler!r}: one of {self.SAMPLERS}')
        return self.sampler

    def _dpmpp_steps(self, clip, cond_scale=1., first=0):
        """the DPM-Solver++ 2M loop as a list of (time, DmhStep, 0), over the time pairs of _ddim_steps.  With a_k =
        sqrt(abar[t_k]), s_k = sqrt(1 - abar[t_k]), lam_k = ln(a_k / s_k), h_k = lam_{k+1} - lam_k and e_k = -expm1(-h_k), entry
        k moves to t_{k+1} by  img' = c1 * img + c0 * x0_k + c2 * x0_{k-1}  (x0: the clamped data prediction, as DDIM's):
        c1 = s_{k+1} / s_k; first order (entry 0, and the last entry that updates: 'lower order final') c0 = a_{k+1} e_k,
        c2 = 0; second order, r = h_{k-1} / h_k: c0 = a_{k+1} e_k (1 + 1/(2r)), c2 = -a_{k+1} e_k / (2r).  float64 from the
        fp32 alphas_cumprod buffer.  The entry with time_next < 0 returns x0 (MODE_LAST).  first (sample_from:
        schedule.start_entry): the solver over the time pairs from ``first`` on — its entry 0, first order, is pair ``first``."""
        host = self._host()
        abar = host['alphas_cumprod'].double()
        pairs = ddim_pairs(self.num_timesteps, self.sampling_timesteps)
        if any(tn >= t for t, tn in pairs):
            raise ValueError(f'dpmpp_2m: the sampling times {[t for t, _ in pairs]} are not strictly decreasing '
                             f'(sampling_timesteps = {self.sampling_timesteps} of {self.num_timesteps}): a step of width 0')
        pairs = pairs[first:]

        def a_s_lam(t):
            a, sg = math.sqrt(float(abar[t])), math.sqrt(1. - float(abar[t]))
            return a, sg, math.log(a / sg)
        updating = [k for k, (_, tn) in enumerate(pairs) if tn >= 0]
        steps, h_prev = [], None
        for k, (time, time_next) in enumerate(pairs):
            if time_next < 0:
                steps.append((time, self._step(host, time, ops.MODE_LAST, clip, cond_scale=cond_scale), 0))
                continue
            (_, s0, l0), (a1, s1, l1) = a_s_lam(time), a_s_lam(time_next)
            h = l1 - l0
            e = -math.expm1(-h)
            if k == 0 or k == updating[-1]:
                c = (a1 * e, s1 / s0, 0.)
            else:
                r = h_prev / h
                c = (a1 * e * (1. + 1. / (2. * r)), s1 / s0, -a1 * e / (2. * r))
            h_prev = h
            steps.append((time, self._step(host, time, ops.MODE_MULTISTEP, clip, c, cond_scale), 0))
        return steps

    def _sampler_steps(self, clip, cond_scale=1., stays=0, first=0):
        """the step list of the selected sampler (stays: _ddim_steps; the multistep solver has none: _check_known; first: the
        time pairs from ``first`` on)"""
        if self._check_sampler() == 'dpmpp_2m':
            if stays:
                raise ValueError(f"{stays} stay entries with sampler = 'dpmpp_2m': its history has no meaning across a stay")
            return self._dpmpp_steps(clip, cond_scale, first)
        return self._ddim_steps(clip, cond_scale, stays, first)

    # OPT-IN, through cfg.GaussianDiffusion.sample_known only (sample() knows none of it: every existing result, launch, RNG draw
    # and graph key stays what it is).  sample_known(known, known_mask, ...) keeps the elements of the image pair that known_mask
    # marks and generates the rest around them (include/dmhomo_hip_known.h has the definition): at every entry of the time list
    # the logits the update would read — behind flow_guidance / pag_scale, apg_eta or photo_guidance where those are on — are
    # replaced by K = 2 * known - 1 on the kept elements (dmh_known_blend, a select) and go through the existing step and threshold
    # kernels as a conditional output without a null pass; behind the last entry's unnormalise the kept elements are overwritten
    # with ``known`` itself, so they — and their bytes in a record — come back bit for bit.  known_resample = r >= 1: RePaint's
    # harmonisation with jump length 1 (Lugmayr et al. 2022): r - 1 "stay" entries t -> t in front of every entry (_stay_coef), r
    # times the network passes; at r = 1 the generator is consumed exactly as by sample().  score_known: the call leaves
    # last_known_error (B,) float64, the mean squared difference over a sample's kept elements between the last entry's own
    # logits and K (dmh_known_error): how far the model's final prediction is from the pixels it was told to keep.  Refused with
    # another objective than pred_x0 (the overwrite acts on the predicted pair), with clip_mode = 'dynamic' (the threshold's
    # division would move kept pixels), with guidance_rescale > 0 (it rescales a blend the overwrite replaces) and, at r > 1, with
    # sampler = 'dpmpp_2m' (its history has no meaning across a stay).  What it does to samples of trained weights has not been
    # measured.  The unconditional class does not have it.
    known_resample = 1
    score_known = False

    def _check_known(self):
        """-> stays = known_resample - 1 of a sample_known call, after the refusals"""
        r = self.known_resample
        if isinstance(r, bool) or not isinstance(r, int) or r < 1:
            raise ValueError(f'known_resample = {r!r}: an int >= 1')
        if self.objective != 'pred_x0':
            raise ValueError(f'sample_known with objective = {self.objective!r}: the overwrite acts on the predicted image pair, '
                             f'which the network returns under pred_x0 only')
        if self._check_clip_mode() == 'dynamic':
            raise ValueError("sample_known with clip_mode = 'dynamic': the threshold's division would move the kept pixels")
        if self._check_guidance_rescale() > 0.:
            raise ValueError(f'sample_known together with guidance_rescale = {self.guidance_rescale!r}: the rescale works on the '
                             f'blend that the overwrite replaces')
        if r > 1 and self._check_sampler() == 'dpmpp_2m':
            raise ValueError(f"known_resample = {r!r} with sampler = 'dpmpp_2m': its history has no meaning across a stay")
        return r - 1

    # OPT-IN, 'static' by default (every existing result stays what it is).  'dynamic': where a step of the conditional
    # class's sample() clamps x_start to [-1, 1], it instead takes, per sample, s = the ``dynamic_threshold_percentile``-th
    # percentile of |x_start| over the sample's C*H*W values, clamps to [-max(1, s), max(1, s)] and divides by max(1, s)
    # (dynamic thresholding: Saharia et al. 2022, "Imagen", 2.3; 0.995 is that paper's value; the reference has none).  Under
    # classifier-free guidance the prediction leaves the data range and the static clamp saturates it (62-73 % of
    # x_start at cond_scale 3 on the test weights); this is the remedy the DPM-Solver++ paper recommends for guided sampling.
    # A sample whose percentile is <= 1 gets the static clamp, bit for bit.  The percentile is an exact order statistic with
    # torch.quantile's linear interpolation (dmh_row_quantile_abs).  What it does to samples of trained weights has not been
    # measured.  The unconditional class refuses it (ddpm.GaussianDiffusion.sample).
    clip_mode = 'static'
    CLIP_MODES = ('static', 'dynamic')
    dynamic_threshold_percentile = 0.995

    def _check_clip_mode(self):
        if self.clip_mode not in self.CLIP_MODES:
            raise ValueError(f'unknown clip_mode {self.clip_mode!r}: one of {self.CLIP_MODES}')
        p = self.dynamic_threshold_percentile
        if not (isinstance(p, (int, float)) and 0. < p <= 1.):
            raise ValueError(f'dynamic_threshold_percentile = {p!r}: a number in (0, 1]')
        return self.clip_mode

    # OPT-IN, 0. by default (every existing result stays what it is).  phi in (0, 1]: rescaled classifier-free guidance (Lin et
    # al. 2024, "Common Diffusion Noise Schedules and Sample Steps are Flawed", 3.4; the reference has none) in the conditional
    # class's sample(): per sample and step the guided blend null + (cond - null) * cond_scale is multiplied by g = 1 + phi *
    # (std(cond) / std(blend) - 1), which brings it back towards the standard deviation of the conditional output — the remedy
    # for the CAUSE of the saturation that clip_mode = 'dynamic' treats at x_start (a cosine schedule has zero terminal SNR, the
    # regime that paper describes; its value is 0.7).  The factor comes from fp64 row moments (dmh_guidance_factor); a sample
    # whose cond equals its null gets g == 1 exactly.  It takes effect only where the network returns a null pass (cond_scale
    # != 1), with both samplers and both clip modes.  What it does to samples of trained weights has not been measured.  The
    # unconditional class refuses it (ddpm.GaussianDiffusion.sample).
    guidance_rescale = 0.

    def _check_guidance_rescale(self):
        phi = self.guidance_rescale
        if isinstance(phi, bool) or not (isinstance(phi, (int, float)) and 0. <= phi <= 1.):
            raise ValueError(f'guidance_rescale = {phi!r}: a number in [0, 1]')
        return float(phi)

    # OPT-IN, None by default (every existing result, launch and graph key stays what it is).  (lo, hi) with 0 <= lo <= hi <= 1:
    # limited-interval guidance (Kynkaanniemi et al. 2024, "Applying Guidance in a Limited Interval Improves Sample and
    # Distribution Quality in Diffusion Models"; the reference has none) in the conditional class's sample(): the entry of the
    # sampling loop at timestep t is guided iff lo <= u <= hi, u = t / (num_timesteps - 1) in float64 (u = 1: pure noise).  A guided
    # entry is what every entry is without the switch; an unguided one is the same entry at cond_scale == 1: the conditional pass
    # alone (class-dropout draw included, so the generator is consumed identically), no blend, no guidance_rescale; clip_mode and
    # the solver update are unchanged.  The null pass of an unguided entry is not computed: B UNet rows instead of 2B.  The
    # replayed loop keeps its ONE captured step: a per-entry flag table next to the step table gates the row lists of the network
    # (dmh_rows_gated) and copies cond over null behind it (dmh_guidance_gate), so changing the interval never captures again.
    # With cond_scale == 1 it has no effect.  (The paper states its bounds in sigma; with sigma(t) = sqrt(1 / alphas_cumprod[t] -
    # 1), u = the t whose sigma meets the bound, over num_timesteps - 1.)  What it does to samples of trained weights has not been
    # measured.  The unconditional class refuses it (ddpm.GaussianDiffusion.sample).
    guidance_interval = None

    def _check_guidance_interval(self):
        gi = self.guidance_interval
        if gi is None:
            return None
        ok = isinstance(gi, (tuple, list)) and len(gi) == 2 and \
            all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in gi)
        if not (ok and 0. <= gi[0] <= gi[1] <= 1.):
            raise ValueError(f'guidance_interval = {gi!r}: None, or a pair (lo, hi) of numbers with 0 <= lo <= hi <= 1')
        return float(gi[0]), float(gi[1])

    # OPT-IN, None by default (every existing result, launch, RNG draw and graph key stays what it is).  pag_scale = s, a finite
    # number >= 0: perturbed-attention guidance (Ahn et al. 2024, "Self-Rectifying Diffusion Sampling with Perturbed-Attention
    # Guidance"; the reference has none) in the conditional class's sample().  It needs no label, no null class and no retraining:
    # with the switch on the network also runs a perturbed pass p — the conditional pass with the attention map of mid_attn, the
    # UNet's one full self-attention, replaced by the identity (dmh_attention_pag) — in the same launch sequence
    # (Unet._cond_null_pag: 3B rows instead of 2B, resp. 2B instead of B), and dmh_pag_shift moves the logits by e = s * (c - p) in
    # front of everything else: the blend behind it is n + cond_scale * (c - n) + s * (c - p) (include/dmhomo_hip.h has the
    # definition; the update is linear, so it is the paper's formula under every objective).  guidance_rescale, apg_eta,
    # photo_guidance, both clip modes, both samplers, every objective, dedup_dropped_rows and the captured step work on the shifted
    # logits unchanged; no random draw is added (pag_scale = 0 gives the samples of None at the cost of the extra pass).  Refused
    # with flow_guidance (a fourth pass is out of scope), with guidance_interval (the gated row lists have no definition for a
    # third pass) and with cfg_mode = 'streams'.  The LinearAttention blocks are not perturbed.  model_predictions and
    # forward_with_cond_scale do not know it.  What it does to samples of trained weights has not been measured.  The
    # unconditional class refuses it (ddpm.GaussianDiffusion.sample).
    pag_scale = None

    def _check_pag(self):
        """-> None (off), or s = pag_scale as a float"""
        s = self.pag_scale
        if s is None:
            return None
        if not (isinstance(s, (int, float)) and not isinstance(s, bool) and 0. <= s < float('inf')):
            raise ValueError(f'pag_scale = {s!r}: None (off), or a finite number >= 0')
        fg = getattr(self, 'flow_guidance', None)
        if fg is not None:
            raise ValueError(f'pag_scale = {s!r} together with flow_guidance = {fg!r}: a fourth pass is not defined; use one '
                             f'of the two')
        if self._check_guidance_interval() is not None:
            raise ValueError(f'pag_scale = {s!r} together with guidance_interval = {self.guidance_interval!r}: the gated row '
                             f'lists have no definition for a third pass')
        if getattr(self.model, 'cfg_mode', None) == 'streams':
            raise ValueError(f"pag_scale = {s!r} together with cfg_mode = 'streams': the perturbed pass is defined for cfg_mode "
                             f"= 'batched' only")
        return float(s)

    def _guided_entries(self, times, cond_scale):
        """which entries of a sampling loop over ``times`` are guided under guidance_interval: a list of bools, or None where
        the switch does nothing (no interval, or cond_scale == 1: no null pass to leave out) — the loops as they were"""
        gi = self._check_guidance_interval()
        if gi is None or cond_scale == 1:
            return None
        span = float(max(self.num_timesteps - 1, 1))
        return [gi[0] <= float(t) / span <= gi[1] for t in times]

    @staticmethod
    def _quantile_rank(p, n):
        """percentile p in (0, 1] of n values -> (k, frac): rank = p * (n - 1) in double, k = floor(rank), frac = the fp32
        value of rank - k; the quantile is v[k] + frac * (v[k+1] - v[k]) over the sorted values (v[k+1] unread at frac == 0)"""
        import ctypes
        n = int(n)
        if n < 1 or not 0. < p <= 1.:
            raise ValueError(f'_quantile_rank: p = {p!r} in (0, 1] and n = {n} >= 1 expected')
        rank = float(p) * (n - 1)
        k = int(math.floor(rank))
        frac = ctypes.c_float(rank - k).value
        if frac >= 1.:                                       # (rank - k rounds up to 1 in fp32: the next order statistic)
            k, frac = k + 1, 0.
        return k, frac

    # hip_graph = True: ONE denoise step of a sampling loop (every kernel of it, on however many HIP streams the network
    # uses) is captured into a HIP graph and replayed once per step; the last step (no noise draw, plus the unnormalise) is
    # a second graph in the same memory pool.  The step's coefficients and timestep come from device tables
    # (ops.step_table) that a cursor kernel at the end of the step advances (dmh_sampler_seek), so the same graph serves
    # every step and any step count, the capture costs one step, and the host queues replay k + 1 while replay k runs.
    # Same kernels, same order, same generator stream (torch's Philox offsets are graph inputs; the keyed generator's draw
    # index lives in device memory): results are bitwise those of the eager loop, the capturing call included — the eager
    # warm-up in front of the captures runs with the generator state put back afterwards.  Captures are kept in a small
    # least-recently-used cache (``graph_cache_size`` entries, each with its own graphs, memory pool and static buffers),
    # keyed on everything they bake in: a job that alternates batch shapes — the short last batch of every epoch of
    # scripts/dgm_sample.py's loader, two samplers sharing one model — captures each shape once, not once per
    # alternation.  A miss first drops the entries of replaced weights, schedules or devices: they can never hit again.
    # Off by default; bench.py switches it on for the conditional sampler.
    hip_graph = False
    graph_cache_size = 4
    graph_captures = 0                   # captures made by this object so far (tests count them)

    def _replay_captured(self, shape, device, key, tables, buffers, fill, first=0):
        """Run the sampling loop through the cache of captured steps (above) -> the last step's output (a copy).
        key: what the class bakes into its captures (weights, schedule and device are added here).  tables() -> (steps,
        times, draws), the loop's entries in order (built on a miss only).  buffers(st, times, draws): puts the class's
        static buffers into the new entry ``st`` (which already holds the step table, 'img' and 'tcond') and returns its
        step bodies (mid, last): mid one step in place on st['img'], last the last step, returning the output.
        fill(st): writes this call's static inputs (and the first noise draw into st['img']) in front of the replay.
        first: the entry of the table the replay starts at (sample_from under 'ddim': the capture and its table are sample()'s)."""
        self.model._engine.ensure_prepared()
        self._host()                                         # (host mirrors cached before any capture)
        live = (self.model._engine._sig, self.__dict__['_host_cache'][0], str(device))
        key = tuple(key) + live
        cache = self.__dict__.setdefault('_graph_states', OrderedDict())
        st = cache.get(key)
        if st is not None:
            cache.move_to_end(key)
        else:
            for k in [k for k in cache if k[-len(live):] != live]:
                del cache[k]                                 # captures of replaced weights / schedules / devices
            steps, times, draws = tables()
            table, tt, cursor, cur = ops.step_table(steps, times, device)
            st = {'key': key, 'table': table, 'times': tt, 'cursor': cursor, 'cur': cur, 'nsteps': len(steps),
                  'img': torch.zeros(shape, device=device),
                  'tcond': torch.zeros((shape[0],), device=device, dtype=torch.long)}
            mid, last = buffers(st, times, draws)
            # eager warm-up of both bodies on a side stream (first-launch work: LDS attributes, side streams), as
            # torch.cuda.graphs asks for, then the captures; the generator state is put back afterwards, so the capturing
            # call consumes exactly what an eager call would
            rng_state = self.rng.snapshot(device)
            ops.sampler_seek(cursor, 0, table, tt, cur, st['tcond'])
            side = torch.cuda.Stream(device=device)
            side.wait_stream(torch.cuda.current_stream())
            tab = st.get('ss_tab')                           # cfg: the (scale, shift) tables Unet._run reads while the
            if tab is not None:                              # step bodies run
                self.model.__dict__['_ss_tab'] = tab
            try:
                with torch.cuda.stream(side):
                    mid()
                    ops.sampler_seek(cursor, len(steps) - 1, table, tt, cur, st['tcond'])   # last() runs on the last entry
                    last()
                torch.cuda.current_stream().wait_stream(side)
                g_mid = torch.cuda.CUDAGraph()
                with graph_capture(g_mid):
                    mid()
                g_last = torch.cuda.CUDAGraph()
                with graph_capture(g_last, pool=g_mid.pool()):
                    st['out'] = last()
            finally:
                self.model.__dict__.pop('_ss_tab', None)
            self.rng.restore(rng_state, device)
            st['graph'], st['graph_last'], st['mid'] = g_mid, g_last, mid       # (mid: the step body, for tools that inspect it)
            cache[key] = st
            self.graph_captures = self.graph_captures + 1
            while len(cache) > max(int(self.graph_cache_size), 1):
                cache.popitem(last=False)                    # least recently used: its graphs, pool and buffers go with it
        self.__dict__['_graph_state'] = st                   # (the entry this call replays)
        fill(st)
        first = int(first)
        if not 0 <= first < st['nsteps']:
            raise ValueError(f'_replay_captured: first = {first} of {st["nsteps"]} entries')
        ops.sampler_seek(st['cursor'], first, st['table'], st['times'], st['cur'], st['tcond'])
        for _ in range(st['nsteps'] - 1 - first):
            st['graph'].replay()
        st['graph_last'].replay()
        return st['out'].clone()
