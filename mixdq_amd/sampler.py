"""The sampling loop around the UNet, on the device: embeddings and noise in, latents out.

    Sampler(unet, kind, n_steps, guidance_scale=0.0, spacing=None).sample(noise, encoder_hidden_states, ...)

Euler, Euler-ancestral and LCM updates of an epsilon-predicting model are one affine map per step,

    x' = a * x + b * e + c * n,        UNet input of the next step = f16(x' * s_next),

so a schedule is a table `coef[n_steps][4] = (a, b, c, s_next)` plus the timesteps; `schedule()` computes both in
float64 with numpy (no diffusers import) and stores them as FP32.  One kernel (mixdq_sampler_step, csrc/sampler.hip)
applies guidance and that map, writes the next UNet input and advances a step index and the UNet's timestep ON THE
DEVICE; `Sampler` captures the UNet forward + that step once into a hipGraph and replays it n_steps times with
nothing from the host in between.  The FP32 arithmetic, rounding by rounding, is include/mixdq_math.h; its numpy
restatement is tests/sampler_ref.py.

Image-to-image starts the same loop at a later step: `img2img_start(n_steps, strength)` is the first step index t0,
`Schedule.start(t0)` the scalars that noise the encoded image to that step's level, and
`sample(..., init_latents=z, strength=s)` sets the device step state to t0 and replays the SAME graph n_steps - t0
times.  `Sampler.img2img` runs VAEEncoder.encode, that loop and VAEDecoder.decode on one stream.

Inpainting (a 4-channel UNet, diffusers' StableDiffusion[XL]InpaintPipeline with num_channels_unet == 4) is the same
loop with one more map per step: after the update, the region the mask keeps is overwritten with the image latents
noised to the NEXT step's level, x = (1 - m) * (p * z + q * noise) + m * x', (p, q) = `Schedule.blend[step]`
(mixdq_sampler_step_masked).  `sample(..., init_latents=z, mask=m)` replays a second captured graph -- the UNet forward
plus that step -- on the same static buffers; `Sampler.inpaint` runs encode, mixdq_mask_to_latent, that loop, decode
and, on request, the uint8 composite with the original image on one stream.

'ddim' is one more such table.  'dpmpp_2m' (DPM-Solver++ 2M, diffusers' DPMSolverMultistepScheduler, optionally with
Karras sigmas) is not an affine map of (x, e, n): from its second step on it also reads the previous step's data
prediction x0 = u * x + v * e.  Its table is `multistep_table`, [n_steps][8] = (u, v, A, B1, B2, D2, s_next, 0); the
Sampler keeps that one extra tensor (`_hist`) and the index of the run's first step (`_first`) on the device beside the
step index, and the captured graphs record mixdq_sampler_step_2m[_masked] instead.  The step at `_first` and the last
one are first-order, so a run never reads what an earlier run left in `_hist`.

`sample(..., seed=)` makes the noise on the device instead of taking it: Philox4x32-10 keyed by a 64-bit seed per image,
counter (element / 4, step, stream), Box-Muller on 24-bit uniforms (include/mixdq_math.h; numpy restatement:
tests/rng_ref.py).  The start noise is one mixdq_randn_f32 launch; the noise of stochastic steps is computed inside
mixdq_sampler_step[_masked]_rng, recorded in graphs of their own that read a static seed buffer.

The inpainting CHECKPOINTS (a 9-channel UNet: unet.cond_channels == 5, diffusers' pipeline with num_channels_unet == 9)
read cat([scaled latents, latent mask, latents of the image with the masked pixels blanked]).  The five conditioning
channels are constant over a run, and a conv is linear in its input channels: `sample(..., cond=c)` computes conv_in's
share of them once per call (unet.cond_term, outside the graph) into one static [R, C0, h, w] buffer, and every captured
step runs the 4-channel conv_in with that buffer as the residual of its epilogue.  The step kernels, the [R, 4, h, w]
input buffer and the four graphs stay as they are; `cond` is orthogonal to init_latents / strength / mask / seed.
`Sampler.inpaint` builds `cond` (VAEEncoder.encode(image, noise, mask=), mixdq_mask_to_latent, mixdq_inpaint_cond_f16),
and runs such a UNet without the blend; `Sampler.inpaint_ext` is inpaint with three more keywords (`inpaint` calls it
with their defaults): `blend=True` keeps the blend as well, `mask_grow` > 0 grows the mask first
(mixdq_mask_dilate_u8), `cond_latent_noise` is the blanked image's posterior noise.  DESIGN.md section 3.30.

InstructPix2Pix (an 8-channel UNet: unet.cond_channels == 4; diffusers' StableDiffusion[XL]InstructPix2PixPipeline) is a
different loop, not just another checkpoint: `Sampler(..., image_guidance_scale=s_I)` runs THREE UNet rows per image --
row blocks in those pipelines' order: text + image, image only, neither -- and every captured graph records
mixdq_sampler_step3, whose guidance is e = e_u + s_T (e_t - e_i) + s_I (e_i - e_u).  The conditioning differs between
the row blocks: the UNSCALED image latents (the posterior's mode) in the first two, zero in the third
(mixdq_ip2p_cond_f16).  `Sampler.instruct` runs VAEEncoder.moments, that launch, the loop from pure noise and
VAEDecoder.decode on one stream.  Everything else -- kinds, masks, seeds, the four graphs, the static buffers -- is
unchanged: 3B rows is simply a batch.  DESIGN.md section 3.32.
"""
import numpy as np

KINDS = ("euler_ancestral", "euler", "lcm")          # the kinds of the first device-side loop (sigma-space or LCM start)
VP_KINDS = ("ddim", "dpmpp_2m")                      # state kept in VP space: init_scale = input_scale0 = s_next = 1
ALL_KINDS = KINDS + VP_KINDS
TRAIN_STEPS = 1000
LCM_ORIGINAL_STEPS = 50
KARRAS_RHO = 7.0
_DEFAULT_SPACING = {"euler_ancestral": "trailing", "euler": "leading", "lcm": "lcm", "ddim": "leading",
                    "dpmpp_2m": "leading"}


def rescale_betas_zero_snr(betas: np.ndarray) -> np.ndarray:
    """diffusers' rescale_betas_zero_snr (Lin et al., algorithm 1) in float64: sqrt(alphas_cumprod) shifted so that its
    last value is 0 and scaled so that its first one stays, turned back into betas.  The last beta is exactly 1."""
    bar_sqrt = np.sqrt(np.cumprod(1.0 - betas))
    first, last = bar_sqrt[0], bar_sqrt[-1]
    bar_sqrt = (bar_sqrt - last) * (first / (first - last))
    bar = bar_sqrt ** 2
    return 1.0 - np.concatenate([bar[:1], bar[1:] / bar[:-1]])


def alphas_cumprod(zero_snr=False) -> np.ndarray:
    """Stable Diffusion's scaled-linear betas: cumprod(1 - linspace(sqrt(0.00085), sqrt(0.012), 1000) ** 2).
    zero_snr: of those betas through rescale_betas_zero_snr -- the last entry is then exactly 0."""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, TRAIN_STEPS, dtype=np.float64) ** 2
    if zero_snr:
        betas = rescale_betas_zero_snr(betas)
    return np.cumprod(1.0 - betas)


def train_sigmas() -> np.ndarray:
    """sqrt((1 - ac) / ac) at the 1000 training timesteps, rising."""
    ac = alphas_cumprod()
    return np.sqrt((1.0 - ac) / ac)


def karras_sigmas(n_steps: int) -> np.ndarray:
    """Karras et al.'s rho = 7 ramp of `n_steps` sigmas between the training schedule's largest and smallest one
    (diffusers' use_karras_sigmas), falling, without the final 0."""
    sig = train_sigmas()
    lo, hi = sig[0] ** (1.0 / KARRAS_RHO), sig[-1] ** (1.0 / KARRAS_RHO)
    return (hi + np.linspace(0.0, 1.0, n_steps) * (lo - hi)) ** KARRAS_RHO


def timesteps(kind: str, n_steps: int, spacing=None, karras=False) -> np.ndarray:
    """The integer training timesteps a run of `n_steps` visits, first (noisiest) first.  karras ('dpmpp_2m' only):
    the timesteps at which the training schedule has the Karras ladder's sigmas, round(interp(log sigma, log
    sigma_train, 0..999)) -- the ladder takes the place of a spacing."""
    if kind not in ALL_KINDS:
        raise ValueError(f"kind must be one of {ALL_KINDS}, not {kind!r}")
    if not 1 <= n_steps <= TRAIN_STEPS:
        raise ValueError("n_steps must be in [1, 1000]")
    if karras:
        if kind != "dpmpp_2m":
            raise ValueError("karras sigmas are for 'dpmpp_2m' only")
        if spacing is not None:
            raise ValueError("karras sigmas take the place of a spacing: leave spacing None")
        t = np.interp(np.log(karras_sigmas(n_steps)), np.log(train_sigmas()), np.arange(TRAIN_STEPS, dtype=np.float64))
        return np.round(t).astype(np.int64)
    spacing = spacing or _DEFAULT_SPACING[kind]
    if kind == "lcm":
        if spacing != "lcm":
            raise ValueError("lcm has its own spacing")
        if n_steps > LCM_ORIGINAL_STEPS:
            raise ValueError("lcm: at most 50 steps")
        origin = (np.arange(1, LCM_ORIGINAL_STEPS + 1) * (TRAIN_STEPS // LCM_ORIGINAL_STEPS) - 1)[::-1]
        idx = np.floor(np.linspace(0, LCM_ORIGINAL_STEPS, n_steps, endpoint=False)).astype(np.int64)
        return origin[idx].astype(np.int64)
    if spacing == "trailing":
        return (np.round(TRAIN_STEPS - np.arange(n_steps) * (TRAIN_STEPS / n_steps)) - 1).astype(np.int64)
    if spacing == "leading":
        return ((np.arange(n_steps) * (TRAIN_STEPS // n_steps))[::-1] + 1).astype(np.int64)
    raise ValueError(f"spacing must be 'trailing' or 'leading', not {spacing!r}")


def img2img_start(n_steps: int, strength: float) -> int:
    """The index of the first step an image-to-image run of `strength` takes out of an `n_steps` schedule: diffusers'
    `get_timesteps`, t_start = max(n_steps - min(int(n_steps * strength), n_steps), 0), the int() of the float
    product as written there.  strength 1.0 is the whole schedule (the image only sets the mean of the start state)."""
    n_steps = int(n_steps)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength must be in (0, 1], not {strength!r}")
    if n_steps < 1:
        raise ValueError("n_steps must be at least 1")
    t0 = max(n_steps - min(int(n_steps * strength), n_steps), 0)
    if t0 >= n_steps:
        raise ValueError(f"strength {strength} leaves no step of {n_steps} (int(n_steps * strength) == 0)")
    return t0


def multistep_table(sigmas) -> np.ndarray:
    """The float64 [n, 8] table of DPM-Solver++ 2M (epsilon prediction, midpoint) for a falling ladder of n + 1 sigmas
    that ends in 0: row i = (u, v, A, B1, B2, D2, s_next, 0).  With alpha = 1 / sqrt(sigma^2 + 1), sigma_hat = sigma *
    alpha (the VP state is x = alpha * x0 + sigma_hat * eps), lambda = -log sigma, h = lambda_{i+1} - lambda_i,
    E = -alpha_{i+1} * expm1(-h) and r = (lambda_i - lambda_{i-1}) / h:
        x0 = u * x + v * eps                     u = 1 / alpha_i, v = -sigma_i
        first order:   x' = A * x + B1 * x0      A = sigma_hat_{i+1} / sigma_hat_i, B1 = E
        second order:  x' = A * x + B2 * x0 + D2 * x0_prev      B2 = E * (1 + 1 / (2 r)), D2 = -E / (2 r)
    Row 0 has no predecessor and the last row steps to sigma 0, where lambda is infinite: both are first-order (B2 =
    B1, D2 = 0), the last one (A, B1) = (0, 1) -- x' = x0.  s_next is 1: a VP state is the UNet's input as it is."""
    sig = np.asarray(sigmas, dtype=np.float64)
    n = len(sig) - 1
    if n < 1 or sig[-1] != 0.0 or not (sig[:-1] > 0).all() or not (np.diff(sig) < 0).all():
        raise ValueError("sigmas must fall strictly from positive values to a final 0")
    alpha = 1.0 / np.sqrt(sig ** 2 + 1.0)
    hat = sig * alpha
    lam = -np.log(sig[:-1])
    tab = np.zeros((n, 8), dtype=np.float64)
    for i in range(n):
        tab[i, 0], tab[i, 1], tab[i, 6] = 1.0 / alpha[i], -sig[i], 1.0
        if i == n - 1:
            tab[i, 2:6] = (0.0, 1.0, 1.0, 0.0)
            continue
        h = lam[i + 1] - lam[i]
        E = -alpha[i + 1] * np.expm1(-h)
        tab[i, 2:6] = (hat[i + 1] / hat[i], E, E, 0.0)
        if i > 0:
            r = (lam[i] - lam[i - 1]) / h
            tab[i, 4:6] = (E * (1.0 + 1.0 / (2.0 * r)), -E / (2.0 * r))
    return tab


def multistep_table_vp(alpha, hat) -> np.ndarray:
    """multistep_table for a v-predicting model, written in the VP pair (alpha, sigma_hat) of every step (n + 1 values
    each, ending in (1, 0)) so that a first step at zero terminal SNR -- alpha_0 = 0, sigma infinite -- forms nothing
    infinite: x0 = u * x + v * m with u = alpha_i, v = -sigma_hat_i, and with lambda = log(alpha / sigma_hat)
        e^-h = (alpha_i / sigma_hat_i) * (sigma_hat_{i+1} / alpha_{i+1}),      E = -alpha_{i+1} * expm1(-h)
    where alpha_i = 0 gives e^-h = 0 and E = alpha_{i+1}.  The step behind such a first one has r = infinity: B2 = E,
    D2 = 0, a first-order row.  Everything else is multistep_table's."""
    alpha, hat = np.asarray(alpha, dtype=np.float64), np.asarray(hat, dtype=np.float64)
    n = len(alpha) - 1
    if (n < 1 or len(hat) != n + 1 or hat[-1] != 0.0 or not (hat[:-1] > 0).all() or not (alpha[1:] > 0).all()
            or alpha[0] < 0 or not (np.diff(hat) < 0).all()):
        raise ValueError("(alpha, sigma_hat) must fall strictly in sigma_hat to a final (alpha > 0, 0)")
    tab = np.zeros((n, 8), dtype=np.float64)
    lam = [np.log(a / s) if a > 0 else None for a, s in zip(alpha[:-1], hat[:-1])]
    for i in range(n):
        tab[i, 0], tab[i, 1], tab[i, 6] = alpha[i], -hat[i], 1.0
        if i == n - 1:
            tab[i, 2:6] = (0.0, 1.0, 1.0, 0.0)
            continue
        E = alpha[i + 1] if lam[i] is None else -alpha[i + 1] * np.expm1(-(lam[i + 1] - lam[i]))
        tab[i, 2:6] = (hat[i + 1] / hat[i], E, E, 0.0)
        if i > 0 and lam[i - 1] is not None:
            r = (lam[i] - lam[i - 1]) / (lam[i + 1] - lam[i])
            tab[i, 4:6] = (E * (1.0 + 1.0 / (2.0 * r)), -E / (2.0 * r))
    return tab


PREDICTION_TYPES = ("epsilon", "v_prediction")


class Schedule:
    """What one (kind, n_steps, spacing) needs: `timesteps` int64 [n]; `sigmas` float64 [n + 1] (euler kinds; ends in
    0); `coef` FP32 [n, 4] = (a, b, c, s_next), computed in float64; `t_table` FP32 [n + 1] (the
    timesteps, then one unused entry the last step's advance reads); `init_scale`: initial state = noise *
    init_scale; `input_scale0`: first UNet input = f16(state * input_scale0); `blend` FP32 [n, 2] = (p, q), computed in
    float64: what the masked step noises the kept region with after step i -- row i < n - 1 the schedulers' add_noise
    at timesteps[i + 1] (`start(i + 1)[:2]`), the last row (1, 0): the kept region ends as the clean image latents.

    'ddim' (diffusers' DDIMScheduler as Stable Diffusion configures it: eta 0, set_alpha_to_one False) is one more
    [n, 4] table.  'dpmpp_2m' (`karras`: the rho = 7 sigma ladder in place of a spacing) is the one kind of `order` 2:
    `coef` is FP32 [n, 8], `multistep_table(sigmas)` rounded, for mixdq_sampler_step_2m; `sigmas` float64 [n + 1].

    prediction_type 'v_prediction' (SD 2.x-768 and the v-prediction fine-tunes): the model returns v = sqrt(ac) * eps -
    sqrt(1 - ac) * x0.  eps = sqrt(1 - ac) * x_vp + sqrt(ac) * v is affine in (state, model output) as every update
    here is, so it folds into the same tables -- only (a, b), or (u, v) of 'dpmpp_2m', differ; the kernels, start(),
    blend and the scales do not.  zero_snr (with 'v_prediction', 'ddim' or 'dpmpp_2m' without karras, and trailing
    spacing only): the betas go through rescale_betas_zero_snr, the first step sits at ac == 0 -- pure noise, start(0)
    == (0, 1, 1) -- and `sigmas` is None ('dpmpp_2m' keeps (alpha, sigma_hat) per step in `vp`; its second row is
    first-order, multistep_table_vp)."""

    def __init__(self, kind, n_steps, spacing=None, karras=False, prediction_type="epsilon", zero_snr=False):
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"prediction_type must be one of {PREDICTION_TYPES}, not {prediction_type!r}")
        vpred = prediction_type == "v_prediction"
        if zero_snr:
            if not vpred:
                raise ValueError("zero_snr needs prediction_type='v_prediction': at ac == 0 the state carries no "
                                 "signal and an epsilon prediction divides by sqrt(ac)")
            if kind not in VP_KINDS or karras:
                raise ValueError("zero_snr needs a state kept in VP space ('ddim', or 'dpmpp_2m' without karras): a "
                                 "sigma-space state is infinite at ac == 0")
            if spacing != "trailing":
                raise ValueError("zero_snr needs spacing='trailing': only then does the first step sit at ac == 0")
        self.kind, self.n_steps = kind, int(n_steps)
        self.prediction_type, self.zero_snr = prediction_type, bool(zero_snr)
        self.timesteps = ts = timesteps(kind, n_steps, spacing, karras)
        self.order = 2 if kind == "dpmpp_2m" else 1
        self.vp = None
        ac = alphas_cumprod(zero_snr) if zero_snr else alphas_cumprod()
        coef = np.zeros((n_steps, 4), dtype=np.float64)
        if kind == "dpmpp_2m" and zero_snr:
            self.sigmas = None
            self.vp = (np.concatenate([np.sqrt(ac[ts]), [1.0]]), np.concatenate([np.sqrt(1.0 - ac[ts]), [0.0]]))
            coef = multistep_table_vp(*self.vp)
            self.init_scale, self.input_scale0 = 1.0, 1.0
        elif kind == "dpmpp_2m":
            self.sigmas = np.concatenate([karras_sigmas(n_steps) if karras else np.sqrt((1.0 - ac[ts]) / ac[ts]), [0.0]])
            coef = multistep_table(self.sigmas)
            if vpred:                               # x0 = alpha x - sigma_hat v; the rest of the table is unchanged
                alpha = 1.0 / np.sqrt(self.sigmas[:-1] ** 2 + 1.0)
                coef[:, 0], coef[:, 1] = alpha, -self.sigmas[:-1] * alpha
            self.init_scale, self.input_scale0 = 1.0, 1.0
        elif kind == "ddim":
            self.sigmas = None
            spacing = spacing or _DEFAULT_SPACING[kind]
            for i, t in enumerate(ts):
                if spacing == "leading":
                    prev = t - TRAIN_STEPS // n_steps
                else:
                    prev = ts[i + 1] if i + 1 < n_steps else -1
                ac_prev = ac[prev] if prev >= 0 else ac[0]          # set_alpha_to_one False: the final alpha is ac[0]
                sa, s1a, sp = np.sqrt(ac[t]), np.sqrt(1.0 - ac[t]), np.sqrt(ac_prev)
                # x0 = (x - s1a e) / sa;  x' = sp x0 + sqrt(1 - ac_prev) e
                if vpred:                           # ... with e = s1a x + sa v: nothing is divided by sa
                    sq = np.sqrt(1.0 - ac_prev)
                    coef[i] = (sp * sa + sq * s1a, sq * sa - sp * s1a, 0.0, 1.0)
                    continue
                coef[i] = (sp / sa, np.sqrt(1.0 - ac_prev) - sp * s1a / sa, 0.0, 1.0)
            self.init_scale, self.input_scale0 = 1.0, 1.0
        elif kind == "lcm":
            self.sigmas = None
            for i, t in enumerate(ts):
                last = i == n_steps - 1
                c_skip = 0.25 / ((10.0 * t) ** 2 + 0.25)
                c_out = 10.0 * t / np.sqrt((10.0 * t) ** 2 + 0.25)
                sa, s1a = np.sqrt(ac[t]), np.sqrt(1.0 - ac[t])
                sp = 1.0 if last else np.sqrt(ac[ts[i + 1]])
                # x0 = (x - s1a e) / sa;  den = c_out x0 + c_skip x;  x' = sp den + sqrt(1 - ac_prev) n
                coef[i] = (sp * (c_out / sa + c_skip), -sp * c_out * s1a / sa,
                           0.0 if last else np.sqrt(1.0 - ac[ts[i + 1]]), 1.0)
                if vpred:                           # x0 = sa x - s1a v
                    coef[i, :2] = (sp * (c_out * sa + c_skip), -sp * c_out * s1a)
            self.init_scale, self.input_scale0 = 1.0, 1.0
        else:
            sig = np.concatenate([np.sqrt((1.0 - ac[ts]) / ac[ts]), [0.0]])
            self.sigmas = sig
            for i in range(n_steps):
                s0, s1 = sig[i], sig[i + 1]
                if kind == "euler_ancestral":
                    up = np.sqrt(s1 ** 2 * (s0 ** 2 - s1 ** 2) / s0 ** 2)
                    down = np.sqrt(s1 ** 2 - up ** 2)
                    coef[i] = (1.0, down - s0, up, 1.0 / np.sqrt(s1 ** 2 + 1.0))
                else:
                    coef[i] = (1.0, s1 - s0, 0.0, 1.0 / np.sqrt(s1 ** 2 + 1.0))
                if vpred:                           # e = s0 / (s0^2 + 1) x + v / sqrt(s0^2 + 1), x the sigma-space state
                    delta = coef[i, 1]
                    coef[i, :2] = (1.0 + delta * s0 / (s0 ** 2 + 1.0), delta / np.sqrt(s0 ** 2 + 1.0))
            self.init_scale = float(np.sqrt(sig[0] ** 2 + 1.0)) if kind == "euler_ancestral" else float(sig[0])
            self.input_scale0 = float(1.0 / np.sqrt(sig[0] ** 2 + 1.0))
        self.coef64 = coef                      # the table before its FP32 rounding (tests compare it in float64)
        self.coef = coef.astype(np.float32)
        self.t_table = np.concatenate([ts.astype(np.float64), [0.0]]).astype(np.float32)
        self.uses_noise = self.order == 1 and bool((self.coef[:, 2] != 0).any())
        self.blend = np.array([self.start(i + 1)[:2] for i in range(self.n_steps - 1)] + [(1.0, 0.0)],
                              dtype=np.float64).astype(np.float32)

    def start(self, t0: int):
        """(a0, c0, s0) in float64 for a run that starts at step `t0` from latents z: state = a0 * z + c0 * noise (the
        schedulers' add_noise at timesteps[t0]), first UNet input = f16(state * s0) (their scale_model_input).
        Euler kinds: (1, sigmas[t0], 1 / sqrt(sigmas[t0]^2 + 1)); lcm and ddim: (sqrt(ac), sqrt(1 - ac), 1) at
        timesteps[t0]; dpmpp_2m: the same two in terms of its own sigma, (alpha, sigma * alpha, 1) at sigmas[t0]."""
        if not 0 <= t0 < self.n_steps:
            raise ValueError(f"t0 must be in [0, {self.n_steps}), not {t0}")
        if self.kind in ("lcm", "ddim"):
            ac = (alphas_cumprod(True) if self.zero_snr else alphas_cumprod())[self.timesteps[t0]]
            return float(np.sqrt(ac)), float(np.sqrt(1.0 - ac)), 1.0
        if self.vp is not None:
            return float(self.vp[0][t0]), float(self.vp[1][t0]), 1.0
        sig = self.sigmas[t0]
        if self.kind == "dpmpp_2m":
            alpha = 1.0 / np.sqrt(sig ** 2 + 1.0)
            return float(alpha), float(sig * alpha), 1.0
        return 1.0, float(sig), float(1.0 / np.sqrt(sig ** 2 + 1.0))


def schedule(kind, n_steps, spacing=None, karras=False, prediction_type="epsilon", zero_snr=False) -> Schedule:
    return Schedule(kind, n_steps, spacing, karras, prediction_type, zero_snr)


def seed_tensor(seed, B, device):
    """`seed` as the int64 [B] tensor on `device` whose bits, read as unsigned, are the per-image seeds: a Python int in
    [0, 2^64) -- image b takes (seed + b) mod 2^64; a sequence of B such ints; or an int64 [B] tensor on `device`, taken
    as it is (no host involvement)."""
    import torch
    if torch.is_tensor(seed):
        if not (seed.dtype == torch.int64 and tuple(seed.shape) == (B,) and seed.device == torch.device(device)):
            raise RuntimeError(f"seed: a tensor should be int64 of shape [{B}] on {device}")
        return seed
    if isinstance(seed, int) and not isinstance(seed, bool):
        vals = [seed + b for b in range(B)]
        if not 0 <= seed < 2 ** 64:
            raise RuntimeError("seed: an int should be in [0, 2^64)")
    else:
        vals = list(seed)
        if len(vals) != B or not all(isinstance(v, int) and 0 <= v < 2 ** 64 for v in vals):
            raise RuntimeError(f"seed: a sequence should hold {B} ints in [0, 2^64)")
    vals = [v % 2 ** 64 for v in vals]
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v for v in vals], dtype=torch.int64).to(device)


class Sampler:
    """`n_steps` of `kind` ('euler_ancestral': SDXL-Turbo, trailing spacing; 'euler': SDXL base, leading spacing with
    offset 1, `spacing='trailing'` selectable; 'lcm': SD 1.5 LCM-LoRA; 'ddim' and 'dpmpp_2m': the non-distilled
    checkpoints, leading spacing with offset 1, 'trailing' selectable, `karras=True`: 'dpmpp_2m' on the Karras sigma
    ladder) around `unet`, a mixdq_amd UNet on the GPU.

    guidance_scale > 1: classifier-free guidance -- the UNet runs at 2B rows, `encoder_hidden_states` (and the
    tensors of `added_cond_kwargs`) carry the B unconditional rows first, then the B conditional ones, as diffusers'
    pipelines concatenate them; otherwise the UNet runs at B rows.

    The first sample() captures ONE step -- the UNet forward, then mixdq_sampler_step -- into a hipGraph on static
    buffers; every sample() copies its inputs in, resets the device step state and replays that graph n_steps
    times: no host synchronisation, host write or eager kernel between the replays.  Inputs of another shape need
    another Sampler.  The first sample(mask=...) captures a SECOND graph on the same buffers -- the UNet forward, then
    mixdq_sampler_step_masked -- which shares the first one's memory pool (neither keeps a tensor alive between
    replays, and they never run concurrently); the plain graph is not touched, and one Sampler serves text-to-image,
    image-to-image and masked calls in any order.

    sample(seed=...) makes the noise on the device (mixdq_randn_f32; the counter layout: include/mixdq_math.h).  Where
    the schedule adds noise per step, the first seeded call captures one more graph -- the UNet forward, then
    mixdq_sampler_step[_masked]_rng, which computes that noise in registers from a static seed buffer -- on the same
    static buffers and in the same memory pool; calls with and without `seed` alternate in any order, every seed
    replays the same graph, and the [n_steps, ...] noise buffer exists only once a call without `seed` was made.

    image_guidance_scale (a number; None: everything above): InstructPix2Pix.  The UNet runs at 3B rows whatever the
    two scales are, and `encoder_hidden_states` (and the tensors of `added_cond_kwargs`) carry them in diffusers'
    InstructPix2Pix order, cat([prompt, negative, negative]): B rows with text + image, B with the image only, B with
    neither -- NOT the two-row order, where the unconditional rows come first.  `cond` follows the same blocks
    (_C.ip2p_cond).  Every captured graph then records mixdq_sampler_step3 with both scales:
    e = e_u + guidance_scale * (e_t - e_i) + image_guidance_scale * (e_i - e_u).

    prediction_type / zero_snr: Schedule's keywords -- 'v_prediction' for SD 2.x-768 and the v-prediction fine-tunes
    (other numbers in the same tables: no kernel differs), zero_snr with it for checkpoints trained on
    rescale_betas_zero_snr ('ddim' or 'dpmpp_2m', spacing='trailing').  guidance_rescale (phi in [0, 1]; diffusers'
    argument of that name, Lin et al. 2023): with a value > 0 every captured graph records mixdq_sampler_step_rescaled in
    the place of the bindings above -- per image the guided output is multiplied by 1 + phi * (std(text-conditioned
    output) / std(guided output) - 1) over all C * H * W elements (1 where a standard deviation is 0) before the
    update; its workspace is one more static buffer.  It needs two or three rows per image (one row: ValueError).  With
    0, exactly the bindings above are recorded.

    controlnet (a mixdq_amd.controlnet.ControlNet, or a list of up to 4): every captured graph then records, in this
    order, each ControlNet's forward on the UNet's own static inputs, the UNet with control= (one mixdq_control_add_f16
    launch over all skips, the scales read from a static [K, n_steps] table at the device-side step) and the step binding
    it recorded before.  sample(control=, control_scale=, control_start=, control_end=) then REQUIRES control= and
    rewrites the hint terms and the table per call, outside the graph: one graph per mode serves every scale and
    guidance window.  A ControlNet's forward still runs while its window is closed (a captured graph cannot branch);
    only its residuals' loads are saved.  Not with three rows per image (ValueError).  Without controlnet= a Sampler
    captures exactly what it captured before, and refuses control=."""

    def __init__(self, unet, kind, n_steps, guidance_scale=0.0, spacing=None, karras=False, *,
                 image_guidance_scale=None, prediction_type="epsilon", zero_snr=False, guidance_rescale=0.0,
                 controlnet=None):
        self.unet = unet
        self.schedule = Schedule(kind, n_steps, spacing, karras, prediction_type, zero_snr)
        self.kind, self.n_steps = kind, int(n_steps)
        self.guidance_scale = float(guidance_scale)
        self.image_guidance_scale = None if image_guidance_scale is None else float(image_guidance_scale)
        self.rows_per_image = 3 if image_guidance_scale is not None else 2 if self.guidance_scale > 1.0 else 1
        self.guidance_rescale = float(guidance_rescale)
        if not 0.0 <= self.guidance_rescale <= 1.0:
            raise ValueError(f"guidance_rescale must be in [0, 1], not {guidance_rescale!r}")
        if self.guidance_rescale > 0.0 and self.rows_per_image == 1:
            raise ValueError("guidance_rescale compares the guided output with the text-conditioned one: it needs "
                             "guidance (guidance_scale > 1 or image_guidance_scale), and this Sampler runs one row per "
                             "image")
        self._graph = None
        self._graph_masked = None
        self._graph_rng = None
        self._graph_masked_rng = None
        self._seeds = None
        self._start = None
        self._key = None
        self._cond_term = None        # the static [R, C0, h, w] conv_in term of a UNet with conditioning channels
        self.controlnets = []
        if controlnet is not None:
            from mixdq_amd.controlnet import MAX_NETS, ControlNet
            nets = list(controlnet) if isinstance(controlnet, (list, tuple)) else [controlnet]
            if not nets or not all(isinstance(n, ControlNet) for n in nets):
                raise TypeError("Sampler: controlnet should be a mixdq_amd.controlnet.ControlNet or a list of them")
            if len(nets) > MAX_NETS:
                raise ValueError(f"Sampler: at most {MAX_NETS} ControlNets, got {len(nets)}")
            if self.rows_per_image == 3:
                raise ValueError("Sampler: three guidance rows (image_guidance_scale) together with controlnet= are not "
                                 "supported yet")
            self.controlnets = nets
        self._hint_terms = None       # per ControlNet the static [R, C0, h, w] hint term
        self._ctl_scales = None       # the static [K, n_steps] table of conditioning scales

    # ---- static buffers + capture ---------------------------------------------------------------------------
    def _setup(self, noise, encoder_hidden_states, added_cond_kwargs):
        import torch
        from mixdq_amd.quantize_sdxl import _clone_args
        sch, dev = self.schedule, noise.device
        B, C, H, W = noise.shape
        R = B * self.rows_per_image

        def nhwc(*lead, dtype):       # [*lead, C, H, W] logical, channels-last in memory
            nd = len(lead)
            return torch.zeros(*lead, H, W, C, dtype=dtype, device=dev).permute(*range(nd), nd + 2, nd, nd + 1)
        self._nhwc = nhwc
        self._x = nhwc(B, dtype=torch.float32)
        self._in = nhwc(R, dtype=torch.float16)
        self._noise = None            # the [n_steps, ...] step noise: made by the first capture that reads it
        self._coef = torch.from_numpy(sch.coef).to(dev)
        self._t_table = torch.from_numpy(sch.t_table).to(dev)
        self._t = torch.zeros((), dtype=torch.float32, device=dev)
        self._step = torch.zeros(1, dtype=torch.int32, device=dev)
        if sch.order == 2:            # the multistep state: the previous step's x0, and where this run started
            self._hist = nhwc(B, dtype=torch.float32)
            self._first = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.guidance_rescale > 0.0:   # the chunk statistics of mixdq_sampler_step_rescaled: one more static buffer
            from mixdq_amd import _C
            self._rescale_ws = _C.sampler_rescale_workspace(B * C * H * W, C * H * W, dev)
        self._init_scale = torch.tensor(sch.init_scale, dtype=torch.float32, device=dev)
        self._input_scale0 = torch.tensor(sch.input_scale0, dtype=torch.float32, device=dev)
        self._ehs, self._added = _clone_args((encoder_hidden_states, added_cond_kwargs))
        self._key = self._shape_key(noise, encoder_hidden_states, added_cond_kwargs)

    def _step_call(self, masked, rng, channels, n):
        """The step binding of a capture and its arguments behind (x, eps), all by name: (fn, kwargs).  The classic
        bindings where they serve; three rows per image or guidance rescale take a flat one, which has every mode's
        operands and leaves those of a mode that is off at None.  Each static buffer is named here, once."""
        from mixdq_amd import _C
        order2, rescaled, n_image = self.schedule.order == 2, self.guidance_rescale > 0.0, n // self._x.shape[0]
        flat = rescaled or self.rows_per_image == 3
        name = ("sampler_step_rescaled" if rescaled else "sampler_step3" if flat else
                "sampler_step" + ("_2m" if order2 else "") + ("_masked" if masked else ""))
        kw = dict(inp=self._in, t_table=self._t_table, step=self._step, timestep=self._t, guidance=self.guidance_scale, n=n)
        kw["table" if flat else "coef8" if order2 else "coef"] = self._coef
        if flat:
            kw["image_guidance"] = self.image_guidance_scale
        if rescaled:
            kw.update(rescale=self.guidance_rescale, workspace=self._rescale_ws, n_image=n_image)
        if rescaled or not flat:                    # (sampler_step3 is three rows by name)
            kw["rows_per_image"] = self.rows_per_image
        if masked:
            kw.update(z=self._z, noise0=self._noise0, mask=self._mask, blend=self._blend, channels=channels)
        if order2:
            kw.update(hist=self._hist, first=self._first)
        elif rng:
            kw.update(seeds=self._seeds, n_image=n_image)
        else:
            kw["noise"] = self._noise
        return getattr(_C, name), kw

    def _capture(self, noise, masked=False, rng=False):
        """Capture one step -- the UNet forward, then mixdq_sampler_step (masked: mixdq_sampler_step_masked, reading the
        static z / noise0 / mask buffers made here; rng: the _rng entry points, reading the static seeds in place of
        the step-noise buffer; three rows per image: mixdq_sampler_step3 with the same operands; _step_call chooses) --
        on the static buffers and return the graph."""
        import torch
        dev = noise.device
        B, C, H, W = noise.shape
        forward = getattr(self.unet.forward, "__wrapped__", self.unet.forward)   # (under hip_graph_opt: the eager one)
        if self.schedule.uses_noise and not rng and self._noise is None:
            self._noise = self._nhwc(self.n_steps, B, dtype=torch.float32)
        if masked and not hasattr(self, "_z"):
            self._z = self._nhwc(B, dtype=torch.float32)
            self._noise0 = self._nhwc(B, dtype=torch.float32)
            self._mask = torch.zeros(B, H, W, dtype=torch.float32, device=dev)
            self._blend = torch.from_numpy(self.schedule.blend).to(dev)
        step_fn, step_kw = self._step_call(masked, rng, C, B * C * H * W)   # chosen once, here, not inside one_step
        self._step_binding = step_fn.__name__       # (the binding the last capture recorded: tests read it)

        cond_kw = {} if self._cond_term is None else {"cond_term": self._cond_term}
        nets = [getattr(n.forward, "__wrapped__", n.forward) for n in self.controlnets]

        def one_step():
            ctl_kw = {}
            if nets:                                # every ControlNet on the UNet's own inputs, then the UNet with control=
                from mixdq_amd.unet import ControlResiduals
                res = [f(self._in, self._t, self._ehs, self._added, hint_term=h) for f, h in zip(nets, self._hint_terms)]
                ctl_kw["control"] = ControlResiduals(res, self._ctl_scales, self._step)
            eps = forward(self._in, self._t, self._ehs, self._added, **cond_kw, **ctl_kw)[0]
            if (eps.dtype != torch.float16 or tuple(eps.shape) != tuple(self._in.shape)
                    or any(a != b for a, b, d in zip(eps.stride(), self._in.stride(), eps.shape) if d > 1)):
                raise RuntimeError("Sampler: the UNet's output is not an FP16 tensor of its input's shape in channels-"
                                   f"last storage (shape {tuple(eps.shape)}, strides {eps.stride()}, {eps.dtype})")
            step_fn(self._x, eps, **step_kw)

        self._reset(noise, None)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(2):
                self._step.zero_()
                one_step()
        torch.cuda.current_stream(dev).wait_stream(side)
        self._step.zero_()
        graph = torch.cuda.CUDAGraph()
        graphs = (self._graph, self._graph_masked, self._graph_rng, self._graph_masked_rng)
        others = [g for g in graphs if g is not None]
        pool = {"pool": others[0].pool()} if others else {}
        with torch.no_grad(), torch.cuda.graph(graph, **pool):
            one_step()
        return graph

    @staticmethod
    def _shape_key(noise, ehs, added):
        return (tuple(noise.shape), noise.device, tuple(ehs.shape), ehs.dtype,
                None if added is None else tuple(sorted((k, tuple(v.shape), v.dtype) for k, v in added.items())))

    def _reset(self, noise, step_noise):
        """State of step 0: x = f32(noise) * init_scale, UNet input = f16(x * input_scale0) in every row block, the
        step index 0, the timestep t_table[0].  Device ops in stream order: nothing here waits for the GPU."""
        import torch
        torch.mul(noise.to(torch.float32), self._init_scale, out=self._x)
        self._start_at(0, (self._x * self._input_scale0).to(torch.float16), step_noise)

    def _start_at(self, t0, first, step_noise):
        """What _reset and _reset_at share: the first UNet input into every row block, the step noise, and the device
        step state at t0."""
        B = first.shape[0]
        for r in range(self.rows_per_image):
            self._in[r * B:(r + 1) * B].copy_(first)
        if self._noise is not None and step_noise is not None:
            self._noise.copy_(step_noise)
        self._step.fill_(t0)
        if self.schedule.order == 2:  # the run's first step is first-order: the history of an earlier run is not read
            self._first.fill_(t0)
        self._t.copy_(self._t_table[t0])

    def _reset_at(self, t0, init_latents, noise, step_noise):
        """State of step t0 of an image-to-image run: x = fl32(fl32(a0 * z) + fl32(c0 * noise)) -- two products and one
        sum, each a torch operation of its own so that none can fuse -- UNet input = f16(fl32(x * s0)) in every row
        block, the step index t0, the timestep t_table[t0].  The scalars travel as launch arguments (rounded to FP32
        there); like _reset, nothing here waits for the GPU."""
        import torch
        a0, c0, s0 = self.schedule.start(t0)
        az = torch.mul(init_latents.to(torch.float32), a0)
        cn = torch.mul(noise.to(torch.float32), c0)
        torch.add(az, cn, out=self._x)
        self._start_at(t0, torch.mul(self._x, s0).to(torch.float16), step_noise)

    # ---- the loop -------------------------------------------------------------------------------------------
    def _set_cond(self, cond, noise):
        """sample(cond=): checked, turned into conv_in's constant term by unet.cond_term (which also re-derives the
        split weights in place after a reload) and copied into the static buffer every captured step reads -- device
        work in stream order, nothing read back."""
        import torch
        cc = int(getattr(self.unet, "cond_channels", 0))
        if cc <= 0:
            if cond is not None:
                raise RuntimeError("Sampler.sample: cond given, but the UNet has no conditioning channels")
            return
        B, _, H, W = noise.shape
        R = B * self.rows_per_image
        if cond is None:
            raise RuntimeError(f"Sampler.sample: this UNet has {cc} conditioning channels: cond is required "
                               "(_C.inpaint_cond of the latent mask and the masked image's latents; _C.ip2p_cond of "
                               "the image's moments for InstructPix2Pix)")
        if not (torch.is_tensor(cond) and cond.device == noise.device and cond.dtype == torch.float16
                and cond.dim() == 4 and cond.shape[0] in (B, R) and cond.shape[1] in (cc, 8)
                and tuple(cond.shape[2:]) == (H, W)):
            raise RuntimeError(f"Sampler.sample: cond should be an FP16 tensor of shape [{B} or {R}, {cc} or 8, {H}, "
                               f"{W}] on noise's device")
        term = self.unet.cond_term(cond)
        if self._cond_term is None:
            self._cond_term = torch.zeros((R, H, W, term.shape[1]), dtype=torch.float16,
                                          device=noise.device).permute(0, 3, 1, 2)
        if term.shape[0] == R:
            self._cond_term.copy_(term)
        else:                                       # B rows: the same conditioning in every row block (guidance)
            for r in range(self.rows_per_image):
                self._cond_term[r * B:(r + 1) * B].copy_(term)

    def _set_control(self, control, scale, start, end, noise, t0):
        """sample(control=...): per ControlNet the hint term (an image goes through net.hint_term, which also re-derives
        the 8-channel conv weights in place after a reload; a term is taken as it is) into its static [R, C0, h, w]
        buffer, B rows repeated into every row block, and the [K, n_steps] scale table of this run
        (controlnet.control_scale_table: diffusers' keep rule over the steps t0 .. n_steps - 1) into the static table --
        copies in stream order, outside the graph, nothing read back."""
        import torch
        K = len(self.controlnets)
        if K == 0:
            if control is not None:
                raise TypeError("Sampler.sample: control given, but this Sampler was built without controlnet=")
            return
        if control is None:
            raise TypeError("Sampler.sample: this Sampler was built with controlnet=: control= (the hint image or "
                            "hint_term of every ControlNet) is required")
        from mixdq_amd.controlnet import control_scale_table
        hints = list(control) if isinstance(control, (list, tuple)) else [control]
        if len(hints) != K:
            raise ValueError(f"Sampler.sample: control should bring one hint per ControlNet ({K}), got {len(hints)}")

        def per_net(v, what):
            vals = list(v) if isinstance(v, (list, tuple)) else [v] * K
            if len(vals) != K:
                raise ValueError(f"Sampler.sample: {what} should be a number or one per ControlNet ({K})")
            return [float(x) for x in vals]
        table = control_scale_table(self.n_steps, t0, per_net(scale, "control_scale"), per_net(start, "control_start"),
                                    per_net(end, "control_end"))
        B, _, H, W = noise.shape
        R = B * self.rows_per_image
        terms = []
        for k, (net, hint) in enumerate(zip(self.controlnets, hints)):
            c0 = net.conv_in.out_channels
            if not (torch.is_tensor(hint) and hint.dim() == 4 and hint.device == noise.device and hint.shape[0] in (B, R)):
                raise RuntimeError(f"Sampler.sample: control[{k}] should be a 4-D tensor of {B} or {R} rows on noise's "
                                   "device: the hint image, or what hint_term(image) returned")
            if hint.dtype == torch.float16 and tuple(hint.shape[1:]) == (c0, H, W):
                term = hint
            elif tuple(hint.shape[2:]) == (8 * H, 8 * W):
                term = net.hint_term(hint)
            else:
                raise RuntimeError(f"Sampler.sample: control[{k}] should be a hint image [{B} or {R}, 3, {8 * H}, {8 * W}] "
                                   f"or an FP16 hint term [{B} or {R}, {c0}, {H}, {W}]")
            terms.append(term)
        if self._hint_terms is None:
            self._hint_terms = [torch.zeros((R, H, W, t.shape[1]), dtype=torch.float16,
                                            device=noise.device).permute(0, 3, 1, 2) for t in terms]
            self._ctl_scales = torch.zeros((K, self.n_steps), dtype=torch.float32, device=noise.device)
        for buf, term in zip(self._hint_terms, terms):
            if term.shape[0] == R:
                buf.copy_(term)
            else:
                for r in range(self.rows_per_image):
                    buf[r * B:(r + 1) * B].copy_(term)
        self._ctl_scales.copy_(torch.from_numpy(table))

    def sample(self, noise, encoder_hidden_states, added_cond_kwargs=None, step_noise=None, *, init_latents=None,
               strength=None, mask=None, seed=None, cond=None, control=None, control_scale=1.0, control_start=0.0,
               control_end=1.0):
        """noise [B, C, H, W] (unit variance; FP32 or FP16), encoder_hidden_states [R, T, D] FP16 (R = B, 2B
        under guidance, or 3B with image_guidance_scale), added_cond_kwargs as the UNet takes them (R rows), step_noise [n_steps, B, C, H, W]: the
        noise each stochastic step adds (required where the schedule has a non-zero c: euler_ancestral and lcm with
        more than one step) -- unless `seed` is given.  Returns the FP32 latents.

        `seed`: a Python int in [0, 2^64) (image b uses (seed + b) mod 2^64), a sequence of B ints, or an int64 GPU
        tensor [B] (taken without host involvement).  The noise is then made on the device by Philox4x32-10 and
        Box-Muller (mixdq_randn_f32; |z| <= 5.77): `noise` may be a shape (B, C, H, W) -- the start noise is stream 0
        of the seeds, on encoder_hidden_states' device -- and step_noise must be None: the steps compute their noise
        (stream 1, counter word = the absolute step index) in registers.  With `seed` and a noise TENSOR only the step
        noise comes from the seed.  Image b's noise depends on its seed and shape only: not on B, its batch position or
        the start step -- and it is not torch's or diffusers' noise for that seed.

        Image-to-image: `init_latents` (FP32 or FP16, noise's shape, multiplied by the VAE's scaling_factor: what
        VAEEncoder.encode returns) together with `strength` in (0, 1].  The run starts at step t0 =
        img2img_start(n_steps, strength) from init_latents noised to that step's level (Schedule.start) and replays
        the same captured graph n_steps - t0 times; step_noise keeps its [n_steps, ...] shape, rows >= t0 are read.
        A Sampler captured by either kind of call serves the other.

        Inpainting: `mask` (FP32 [B, h, w] or [B, 1, h, w] on noise's device, values in [0, 1]: 1 repaints, 0 keeps
        -- what _C.mask_to_latent returns, or a soft mask of the caller's) together with `init_latents`.  After every
        step the kept region is overwritten with init_latents noised with `noise` to the next step's level
        (Schedule.blend; after the last step: init_latents themselves), on the second captured graph.  `strength`
        None then means the whole schedule from pure noise, exactly as a text-to-image call starts (diffusers'
        is_strength_max); otherwise the start is image-to-image's.  The mask does not touch the start state.

        `cond` (required exactly when unet.cond_channels > 0: the 9-channel inpainting checkpoints): FP16 [B or R, Cc
        or 8, h, w] on noise's device -- the latent-resolution mask, then the latents of the image with the masked
        pixels blanked, as _C.inpaint_cond writes them; B rows serve every row block (classifier-free guidance reads the
        same mask and image in both).  It is constant over the run, so its share of conv_in is computed ONCE here
        (unet.cond_term, outside the graph) into a static buffer that every captured step adds in its conv_in epilogue:
        no concatenated 9-channel input exists, the graphs are the four above, and calls with different `cond` replay
        the same graph objects.  Orthogonal to init_latents / strength / mask / seed.  An 8-channel InstructPix2Pix
        UNet takes the image latents here: _C.ip2p_cond(enc.moments(image), rows=3) -- R rows, zero in the third block
        (Sampler.instruct builds it).

        `control` (required exactly when the Sampler was built with controlnet=): per ControlNet the hint image (uint8 /
        FP16 / FP32 [B or R, 3, 8h, 8w] in [0, 1]; uint8: 0..255) or what its hint_term(image) returned; one tensor, or
        a list with one per net.  `control_scale`, `control_start`, `control_end`: diffusers'
        controlnet_conditioning_scale, control_guidance_start and control_guidance_end, numbers or one per net.  They
        fill the static hint buffers and the scale table of this run; calls with other values replay the same graph
        objects.  Orthogonal to everything above (`cond` composes: a ControlNet reads the latent channels)."""
        import torch
        from mixdq_amd.quantize_sdxl import _copy_into
        if control is None and self.controlnets:
            self._set_control(None, control_scale, control_start, control_end, None, 0)      # (raises)
        if control is not None and not self.controlnets:
            self._set_control(control, control_scale, control_start, control_end, None, 0)   # (raises)
        seeds = None
        if seed is not None:
            from mixdq_amd import _C
            if step_noise is not None:
                raise RuntimeError("Sampler.sample: with seed the steps make their own noise: step_noise must be None")
            shape = tuple(noise.shape) if torch.is_tensor(noise) else tuple(int(d) for d in noise)
            if len(shape) != 4:
                raise RuntimeError("Sampler.sample: noise should be a [B, C, H, W] GPU tensor or, with seed, that "
                                   "shape")
            dev = encoder_hidden_states.device
            seeds = seed_tensor(seed, shape[0], dev)
            if self._seeds is None:
                self._seeds = torch.zeros(shape[0], dtype=torch.int64, device=dev)
            if tuple(self._seeds.shape) != (shape[0],) or self._seeds.device != dev:
                raise RuntimeError("Sampler.sample: inputs differ in shape from those the step graph was captured for")
            self._seeds.copy_(seeds)
            if not torch.is_tensor(noise):
                if self._start is None or tuple(self._start.shape) != shape:
                    B, C, H, W = shape
                    self._start = torch.empty((B, H, W, C), dtype=torch.float32, device=dev).permute(0, 3, 1, 2)
                noise = _C.randn(shape, self._seeds, _C.RNG_STREAM_START, 0, out=self._start)
        if not (torch.is_tensor(noise) and noise.is_cuda and noise.dim() == 4):
            raise RuntimeError("Sampler.sample: noise should be a [B, C, H, W] GPU tensor")
        if mask is None:
            if (init_latents is None) != (strength is None):
                raise RuntimeError("Sampler.sample: init_latents and strength go together (both, or neither)")
        else:
            if init_latents is None:
                raise RuntimeError("Sampler.sample: mask requires init_latents (the image whose unmasked region is kept)")
            B, _, H, W = noise.shape
            if not (torch.is_tensor(mask) and mask.device == noise.device and mask.dtype == torch.float32
                    and tuple(mask.shape) in ((B, H, W), (B, 1, H, W))):
                raise RuntimeError(f"Sampler.sample: mask should be an FP32 tensor of shape {(B, H, W)} or "
                                   f"{(B, 1, H, W)} on noise's device")
        t0 = 0
        if init_latents is not None:
            if not (torch.is_tensor(init_latents) and init_latents.device == noise.device
                    and tuple(init_latents.shape) == tuple(noise.shape)
                    and init_latents.dtype in (torch.float32, torch.float16)):
                raise RuntimeError("Sampler.sample: init_latents should be an FP32 or FP16 tensor of noise's shape "
                                   f"{tuple(noise.shape)} on its device")
            if strength is not None:
                t0 = img2img_start(self.n_steps, strength)
        R = noise.shape[0] * self.rows_per_image
        if encoder_hidden_states.shape[0] != R:
            raise RuntimeError(f"Sampler.sample: encoder_hidden_states should have {R} rows")
        rng = seeds is not None and self.schedule.uses_noise
        if self.schedule.uses_noise:                # (rng: the steps make it, and step_noise is None)
            want = (self.n_steps,) + tuple(noise.shape)
            if not rng and (step_noise is None or tuple(step_noise.shape) != want):
                raise RuntimeError(f"Sampler.sample: this schedule needs step_noise of shape {want}")
        elif step_noise is not None:
            raise RuntimeError("Sampler.sample: this schedule adds no noise: step_noise must be None")
        if self._key is None:
            self._setup(noise, encoder_hidden_states, added_cond_kwargs)
        elif self._shape_key(noise, encoder_hidden_states, added_cond_kwargs) != self._key:
            raise RuntimeError("Sampler.sample: inputs differ in shape from those the step graph was captured for")
        self._set_cond(cond, noise)
        self._set_control(control, control_scale, control_start, control_end, noise, t0)
        name = "_graph" + ("_masked" if mask is not None else "") + ("_rng" if rng else "")
        if getattr(self, name) is None:
            setattr(self, name, self._capture(noise, masked=mask is not None, rng=rng))
        graph = getattr(self, name)
        if mask is not None:
            self._z.copy_(init_latents)             # (an FP16 tensor widens exactly)
            self._noise0.copy_(noise)
            self._mask.copy_(mask.reshape(self._mask.shape))
        _copy_into((self._ehs, self._added), (encoder_hidden_states, added_cond_kwargs))
        if init_latents is None or strength is None:
            self._reset(noise, step_noise)
        else:
            self._reset_at(t0, init_latents, noise, step_noise)
        for _ in range(self.n_steps - t0):
            graph.replay()
        return self._x.clone()

    def sample_image(self, vae, noise, encoder_hidden_states, added_cond_kwargs=None, step_noise=None, *, seed=None,
                     cond=None, control=None, control_scale=1.0, control_start=0.0, control_end=1.0):
        """sample(), then `vae.decode` (a mixdq_amd.vae.VAEDecoder, eager or under hip_graph_opt) of its latents on
        the same stream: nothing waits for the GPU in between.  Returns (FP32 latents, FP16 image [B, 3, 8H, 8W]).
        `seed`, `cond` and `control*` as in sample(): with seed `noise` may be the latent shape, and seed -> image is
        this one call."""
        latents = self.sample(noise, encoder_hidden_states, added_cond_kwargs, step_noise, seed=seed, cond=cond,
                              control=control, control_scale=control_scale, control_start=control_start,
                              control_end=control_end)
        return latents, vae.decode(latents)

    def _latent_noise(self, latent_noise, latent_seed, noise, encoder_hidden_states, stream=None):
        """The VAE posterior's noise of img2img / inpaint: `latent_noise` as given; with `latent_seed` (as sample()'s
        seed) stream 2 of those seeds at the latent shape (`stream`: another one -- 3 for the blanked image of a
        9-channel inpainting run); neither: None, the posterior's mode."""
        import torch
        from mixdq_amd import _C
        if latent_noise is not None or latent_seed is None:
            if latent_noise is not None and latent_seed is not None and stream is None:
                raise RuntimeError("Sampler: latent_noise and latent_seed exclude each other")
            return latent_noise
        shape = tuple(noise.shape) if torch.is_tensor(noise) else tuple(int(d) for d in noise)
        return _C.randn(shape, seed_tensor(latent_seed, shape[0], encoder_hidden_states.device),
                        _C.RNG_STREAM_VAE if stream is None else stream, 0)

    def img2img(self, enc, dec, image, noise, encoder_hidden_states, added_cond_kwargs=None, *, strength,
                step_noise=None, latent_noise=None, seed=None, latent_seed=None, cond=None, control=None,
                control_scale=1.0, control_start=0.0, control_end=1.0):
        """Image to image on one stream: `enc.encode(image, latent_noise)` (a mixdq_amd.vae.VAEEncoder; latent_noise
        None: the posterior's mode), sample(init_latents=that, strength=strength), then `dec.decode` (a VAEDecoder) --
        either VAE eager or under hip_graph_opt, nothing waits for the GPU in between.  noise: [B, C, H/8, W/8], what
        is added to the encoded image.  Returns (FP32 latents, FP16 image [B, 3, H, W]).  `seed` as in sample() (noise
        may then be the latent shape); it does not touch the posterior, which stays the mode unless `latent_noise` or
        `latent_seed` (stream 2 of those seeds) is given.  `cond` and `control*` as in sample()."""
        z = enc.encode(image, self._latent_noise(latent_noise, latent_seed, noise, encoder_hidden_states))
        latents = self.sample(noise, encoder_hidden_states, added_cond_kwargs, step_noise, init_latents=z,
                              strength=strength, seed=seed, cond=cond, control=control, control_scale=control_scale,
                              control_start=control_start, control_end=control_end)
        return latents, dec.decode(latents)

    def instruct(self, enc, dec, image, noise, encoder_hidden_states, added_cond_kwargs=None, *, step_noise=None,
                 seed=None, cond_scale=1.0):
        """InstructPix2Pix on one stream: `enc.moments(image)` (a mixdq_amd.vae.VAEEncoder), `_C.ip2p_cond(moments,
        rows=self.rows_per_image, scale=cond_scale)`, sample(noise, ..., cond=that) and `dec.decode` (a VAEDecoder) --
        nothing waits for the GPU in between.  The run starts from PURE noise: the image enters only through `cond`, the
        posterior's mode UNSCALED (cond_scale 1.0: diffusers' pipelines; CosXL-Edit: the VAE's scaling_factor) in the
        text + image and image-only row blocks and zero in the unconditional one.  noise: [B, C, H/8, W/8], or with
        `seed` that shape; encoder_hidden_states / added_cond_kwargs: 3B rows, cat([prompt, negative, negative]).
        Returns (FP32 latents, FP16 image [B, 3, H, W]), as img2img.  A Sampler without image_guidance_scale and
        guidance (rows_per_image == 1) runs the image-conditioned row alone; rows_per_image == 2 is refused: a two-row
        run cannot say which block is unconditioned."""
        from mixdq_amd import _C
        cc = int(getattr(self.unet, "cond_channels", 0))
        if cc <= 0 or cc != int(enc.cfg["latent_channels"]):
            raise RuntimeError(f"Sampler.instruct: the UNet's {cc} conditioning channels are not the VAE's "
                               f"{enc.cfg['latent_channels']} latent channels (an InstructPix2Pix UNet has 2 x latent "
                               "input channels)")
        if self.rows_per_image == 2:
            raise RuntimeError("Sampler.instruct: a two-row run cannot say which block is unconditioned: construct the "
                               "Sampler with image_guidance_scale= (three rows per image)")
        cond = _C.ip2p_cond(enc.moments(image), rows=self.rows_per_image, scale=cond_scale)
        latents = self.sample(noise, encoder_hidden_states, added_cond_kwargs, step_noise, seed=seed, cond=cond)
        return latents, dec.decode(latents)

    def inpaint(self, enc, dec, image, mask, noise, encoder_hidden_states, added_cond_kwargs=None, *, strength=None,
                step_noise=None, latent_noise=None, mask_mode="nearest", composite=False, seed=None, latent_seed=None,
                crop=None, crop_pad=32, mask_blur=0.0, resample="lanczos3"):
        """Inpainting on one stream: `enc.encode(image, latent_noise)`, `_C.mask_to_latent(mask, mask_mode)` (mask at
        image resolution, [B, H, W] or [B, 1, H, W], uint8 / FP16 / FP32: set where repainted; 'nearest' is
        diffusers' downscaling, 'any' repaints every latent whose 8x8 block touches the mask),
        sample(init_latents=that, strength=strength, mask=that), `dec.decode` -- nothing waits for the GPU in between.
        strength None: the whole schedule from pure noise.  Returns (FP32 latents, FP16 image [B, 3, H, W]); with
        composite=True `image` must be uint8 and the second result is uint8: the decoded pixels where the mask is
        set, the input's own bytes elsewhere (vae.composite_uint8).  `seed` / `latent_seed` as in img2img.

        `crop` ("only the masked region"): 'auto' (per image: image.mask_bbox -- the one host read-back -- grown by
        `crop_pad` and brought to the model's aspect by image.crop_region), one integer (x0, y0, x1, y1) or B of them.
        `image` is then uint8 of ANY height and width, `mask` has its size, composite must be True, and `noise` (or
        its shape, with seed) fixes the model size as 8 x its extent.  The window is resized to the model size
        (`resample`: 'bilinear' / 'bicubic' / 'lanczos3'; the mask: bilinear of its binarisation), inpainted there,
        and the decode is resized back and pasted into the window of the untouched original (image.paste) under the
        mask -- blurred by `mask_blur` pixels (image.blur_mask) where that is > 0.  Returns (FP32 latents, uint8
        [B, 3, H, W] at the ORIGINAL size); every pixel outside the window, and every pixel whose paste weight is 0,
        is the input's own byte.  After the tables are uploaded (cached by sizes, boxes and filter) nothing comes from
        the host.

        This is inpaint_ext() with its three further keywords at their defaults (blend=None, mask_grow=0,
        cond_latent_noise=None): on a 4-channel UNet what it always was; on a 9-channel inpainting UNet diffusers' loop
        without the blend, the conditioning built from `image` and `mask`."""
        return self.inpaint_ext(enc, dec, image, mask, noise, encoder_hidden_states, added_cond_kwargs,
                                strength=strength, step_noise=step_noise, latent_noise=latent_noise, mask_mode=mask_mode,
                                composite=composite, seed=seed, latent_seed=latent_seed, crop=crop, crop_pad=crop_pad,
                                mask_blur=mask_blur, resample=resample)

    def inpaint_ext(self, enc, dec, image, mask, noise, encoder_hidden_states, added_cond_kwargs=None, *, strength=None,
                    step_noise=None, latent_noise=None, mask_mode="nearest", composite=False, seed=None,
                    latent_seed=None, crop=None, crop_pad=32, mask_blur=0.0, resample="lanczos3", blend=None,
                    mask_grow=0, cond_latent_noise=None):
        """inpaint() -- same arguments, same results -- with the keywords the inpainting checkpoints and mask growth add.

        `mask_grow` > 0: the mask is replaced by `_C.mask_dilate(mask, mask_grow)` -- grown by that many pixels, a
        square window -- for EVERYTHING in the call: the bounding box of crop='auto', the model-size mask, the blanked
        image, the blur, the composite / paste.  (Front ends' "grow mask by"; any UNet.)

        A UNet with conditioning channels (unet.cond_channels == 1 + the VAE's latent channels: the 9-channel
        inpainting checkpoints) is also given `cond = _C.inpaint_cond(latent mask, enc.encode(image, cond_noise,
        mask=mask))`: the mask and the latents of the image with the masked pixels blanked; cond_noise is
        `cond_latent_noise`, else stream 3 of `latent_seed`, else None (the posterior's mode).  `blend`: whether the
        kept region is also overwritten after every step (the masked graph).  None means True for a 4-channel UNet
        (blend=False is refused there: nothing else would keep the image) and False for a 9-channel one, diffusers'
        behaviour: a plain loop or, with `strength`, an image-to-image one -- with strength None the init image is not
        even encoded.  blend=True on a 9-channel UNet runs the masked graph as well.  On the crop path the blanked
        encode reads the resized window and the resized mask.

        A Sampler built with controlnet= is refused here (sample() asks for control=): the signatures of inpaint and
        inpaint_ext are pinned; a masked ControlNet run is sample(mask=, init_latents=, control=)."""
        import torch
        from mixdq_amd import _C
        if composite and not (torch.is_tensor(image) and image.dtype == torch.uint8):
            raise RuntimeError("Sampler.inpaint: composite=True pastes into the input pixels: image should be uint8")
        cc = int(getattr(self.unet, "cond_channels", 0))
        if blend is None:
            blend = cc == 0
        if not blend and cc == 0:
            raise RuntimeError("Sampler.inpaint: blend=False leaves the image to the UNet's conditioning channels, and "
                               "this UNet has none")
        if cc > 0 and cc != 1 + int(enc.cfg["latent_channels"]):
            raise RuntimeError(f"Sampler.inpaint: the UNet's {cc} conditioning channels are not a mask and the VAE's "
                               f"{enc.cfg['latent_channels']} latent channels")
        if not (isinstance(mask_grow, int) and not isinstance(mask_grow, bool) and 0 <= mask_grow <= 255):
            raise RuntimeError("Sampler.inpaint: mask_grow should be an int in [0, 255]")
        if mask_grow > 0:
            mask = _C.mask_dilate(mask, mask_grow)
        kw = dict(strength=strength, step_noise=step_noise, latent_noise=latent_noise, mask_mode=mask_mode, seed=seed,
                  latent_seed=latent_seed, blend=bool(blend), cond_latent_noise=cond_latent_noise)
        if crop is not None:
            return self._inpaint_crop(enc, dec, image, mask, noise, encoder_hidden_states, added_cond_kwargs,
                                      composite=composite, crop=crop, crop_pad=crop_pad, mask_blur=mask_blur,
                                      resample=resample, **kw)
        latents = self._inpaint_latents(enc, image, mask, noise, encoder_hidden_states, added_cond_kwargs, **kw)
        decoded = dec.decode(latents)
        return latents, (_C.composite_u8(decoded, image, mask) if composite else decoded)

    def _inpaint_latents(self, enc, image, mask, noise, encoder_hidden_states, added_cond_kwargs, *, strength,
                         step_noise, latent_noise, mask_mode, seed, latent_seed, blend, cond_latent_noise, control=None,
                         control_scale=1.0, control_start=0.0, control_end=1.0):
        """The model-size part of inpaint(): the encodes, the latent mask, the conditioning, the loop."""
        from mixdq_amd import _C
        m = _C.mask_to_latent(mask, mask_mode)
        cond = None
        if int(getattr(self.unet, "cond_channels", 0)) > 0:
            cond_noise = self._latent_noise(cond_latent_noise, latent_seed, noise, encoder_hidden_states,
                                            stream=_C.RNG_STREAM_COND)
            cond = _C.inpaint_cond(m, enc.encode(image, cond_noise, mask=mask))
        z = None
        if blend or strength is not None:           # (a plain 9-channel run never reads the init image's latents)
            z = enc.encode(image, self._latent_noise(latent_noise, latent_seed, noise, encoder_hidden_states))
        return self.sample(noise, encoder_hidden_states, added_cond_kwargs, step_noise, init_latents=z,
                           strength=strength, mask=m if blend else None, seed=seed, cond=cond, control=control,
                           control_scale=control_scale, control_start=control_start, control_end=control_end)

    def _inpaint_crop(self, enc, dec, image, mask, noise, encoder_hidden_states, added_cond_kwargs, *, composite, crop,
                      crop_pad, mask_blur, resample, **kw):
        """inpaint(crop=...): resize the window to the model size, inpaint there, paste the decode back."""
        import torch
        from mixdq_amd import image as I
        if not (torch.is_tensor(image) and image.dtype == torch.uint8 and image.dim() == 4 and image.shape[1] == 3):
            raise RuntimeError("Sampler.inpaint: crop pastes into the input pixels: image should be uint8 [B, 3, H, W]")
        if not composite:
            raise RuntimeError("Sampler.inpaint: crop returns the pasted pixels: composite should be True")
        if resample not in I.FILTERS:
            raise RuntimeError(f"Sampler.inpaint: resample should be one of {tuple(I.FILTERS)}")
        mask_blur = float(mask_blur)
        if not mask_blur >= 0.0:
            raise RuntimeError("Sampler.inpaint: mask_blur should be >= 0")
        shape = tuple(noise.shape) if torch.is_tensor(noise) else tuple(int(d) for d in noise)
        if len(shape) != 4:
            raise RuntimeError("Sampler.inpaint: noise should be a [B, C, h, w] GPU tensor or, with seed, that shape")
        B, H, W = image.shape[0], image.shape[2], image.shape[3]
        model_hw = (8 * shape[2], 8 * shape[3])
        if not (torch.is_tensor(mask) and mask.dim() in (3, 4) and mask.shape[0] == B
                and tuple(mask.shape[-2:]) == (H, W)):
            raise RuntimeError("Sampler.inpaint: with crop the mask should have the image's batch, height and width")
        if isinstance(crop, str):
            if crop != "auto":
                raise RuntimeError("Sampler.inpaint: crop should be 'auto', one (x0, y0, x1, y1) or one per image")
            boxes = tuple(I.crop_region(bb, (H, W), model_hw, crop_pad) for bb in I.mask_bbox(mask))
        else:
            boxes = I._boxes(crop, B, H, W, "Sampler.inpaint", integer=True)
        mask3 = mask if mask.dim() == 3 else mask[:, 0]
        small = I.resize(image, model_hw, boxes, resample)
        small_mask = I.resize(mask3[:, None], model_hw, boxes, "bilinear", mask=True)[:, 0]
        latents = self._inpaint_latents(enc, small, small_mask, noise, encoder_hidden_states, added_cond_kwargs, **kw)
        decoded = dec.decode(latents)
        soft = mask_blur > 0.0
        return latents, I.paste(decoded, image, I.blur_mask(mask3, mask_blur) if soft else mask3, boxes, resample,
                                soft=soft)
