"""Host side of the DDIM sampler (diffusers DDIMScheduler with SD-1.5's scheduler_config.json: timestep_spacing "leading",
steps_offset 1, set_alpha_to_one False; eta = 0, no sample clipping).  Plain Python on the host schedule: the per-step arithmetic is
cnerf_sd_ddim_step."""


def _leading(num_inference_steps, num_train_timesteps, steps_offset):
    N, T = int(num_inference_steps), int(num_train_timesteps)
    if not 1 <= N <= T:
        raise ValueError(f"num_inference_steps must be in [1, {T}], got {num_inference_steps}")
    step = T // N
    return [i * step + steps_offset for i in reversed(range(N))], step


def ddim_timesteps(num_inference_steps, num_train_timesteps=1000, steps_offset=1):
    """"leading" spacing: (arange(N) * (T // N))[::-1] + offset, e.g. N = 50 -> 981, 961, ..., 1.
    A timestep past the end of the training schedule (N = T with offset 1 gives t = T) is clamped to T - 1: the full-length schedule
    stays usable, its first step then goes from alpha_bar[T - 1] to alpha_bar[T - 1] and leaves the sample's noise level where it is."""
    ts, _ = _leading(num_inference_steps, num_train_timesteps, steps_offset)
    return [min(t, num_train_timesteps - 1) for t in ts]


def ddim_schedule(num_inference_steps, alphas_cumprod, steps_offset=1):
    """-> [(t, alpha_bar_t, alpha_bar_prev)] per step, floats from the host copy of the schedule (no device read).
    prev = t - T // N from the unclamped t; prev < 0 takes alphas_cumprod[0] (set_alpha_to_one = False)."""
    T = len(alphas_cumprod)
    ts, step = _leading(num_inference_steps, T, steps_offset)
    out = []
    for t in ts:
        prev = t - step
        out.append((min(t, T - 1), float(alphas_cumprod[min(t, T - 1)]), float(alphas_cumprod[max(prev, 0)])))
    return out
