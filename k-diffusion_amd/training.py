"""Training-side configuration helpers that the reference keeps in ``k_diffusion/config.py`` (``K.config`` here mirrors the sampling
path's part of that module only, and its public names are pinned).

``make_sample_density(config)`` (config.py:234-268): the sigma density of a model config's ``sigma_sample_density`` section as a
``functools.partial`` over one of ``utils.rand_*``, with the reference's dispatch and defaults; call it as
``sample_density([batch], device=device)`` (train.py:454).
"""
import math
from functools import partial

from . import utils


def make_sample_density(config):
    sd_config = config['sigma_sample_density']
    sigma_data = config['sigma_data']
    kind = sd_config['type']

    def pick(*names, default=None):
        for name in names:
            if name in sd_config:
                return sd_config[name]
        if default is None:
            raise KeyError(names[-1])
        return default()

    if kind == 'lognormal':
        return partial(utils.rand_log_normal, loc=pick('mean', 'loc'), scale=pick('std', 'scale'))
    if kind == 'loglogistic':
        return partial(utils.rand_log_logistic, loc=pick('loc', default=lambda: math.log(sigma_data)), scale=pick('scale', default=lambda: 0.5),
                       min_value=pick('min_value', default=lambda: 0.), max_value=pick('max_value', default=lambda: float('inf')))
    if kind == 'loguniform':
        return partial(utils.rand_log_uniform, min_value=pick('min_value', default=lambda: config['sigma_min']),
                       max_value=pick('max_value', default=lambda: config['sigma_max']))
    if kind in {'v-diffusion', 'cosine'}:
        return partial(utils.rand_v_diffusion, sigma_data=sigma_data, min_value=pick('min_value', default=lambda: 1e-3),
                       max_value=pick('max_value', default=lambda: 1e3))
    if kind == 'split-lognormal':
        return partial(utils.rand_split_log_normal, loc=pick('mean', 'loc'), scale_1=pick('std_1', 'scale_1'), scale_2=pick('std_2', 'scale_2'))
    if kind == 'cosine-interpolated':
        return partial(utils.rand_cosine_interpolated,
                       image_d=pick('image_d', default=lambda: max(config['input_size'])),
                       noise_d_low=pick('noise_d_low', default=lambda: 32),
                       noise_d_high=pick('noise_d_high', default=lambda: max(config['input_size'])),
                       sigma_data=sigma_data,
                       min_value=pick('min_value', default=lambda: min(config['sigma_min'], 1e-3)),
                       max_value=pick('max_value', default=lambda: max(config['sigma_max'], 1e3)))
    raise ValueError('Unknown sample density type')
