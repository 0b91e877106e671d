"""Policy plugin registry -- host-side mirror of `algo/call_algo.py:3-27`.

`call_algo(algo_name, config, mode, device, **kwargs)` lower-cases the name, looks the class up
and returns `cls(config, device)`; `mode` and kwargs are accepted and ignored exactly as the
reference does.  Unknown names raise KeyError like the reference's dict lookup.  Of the baseline
algorithms TD3_BC (`offline_offline/td3_bc.py`), IQL (`offline_offline/iql.py`), DARA (`offline_offline/dara.py`) and IGDF
(`offline_offline/igdf.py`) are built, IQL, DARA and IGDF from a config of their own only: without `lam`, `temp`, `max_step` -- for
DARA also `gaussian_noise_std`, `dara_eta` and, when `dara_eta` is 0, `eta`; for IGDF also `xi`, `importance_weight`, `repr_dim`,
`ensemble_size`, `repr_norm`, `ortho_init`, `info_update_step` -- the constructor raises NotImplementedError.  BOSA
(`offline_offline/bosa.py`) is built in two parts: its VAE stage -- the behaviour and dynamics VAEs, their checkpoints and both
likelihood estimators -- always, its critic / actor stage when config['critic_actor'] is truthy (then `gamma`, `tau`, `actor_lr` and
`critic_lr` are required as well; the optional config['critic_actor_graph'] = 1, read only then, replays that stage's calls as HIP
graphs under rng='device', 0 -- the default -- runs them eagerly, any other value is a ValueError).  A config without one of the seventeen keys the reference reads without defaults (`vae_policy_lr`
... `update_interval`) raises NotImplementedError in the constructor, and so does -- with `critic_actor` unset -- the train() call that
would enter the critic / actor stage.
"""
from .offline_offline.mobody import MOBODY
from .offline_offline.td3_bc import TD3BC
from .offline_offline.iql import IQL
from .offline_offline.dara import DARA
from .offline_offline.igdf import IGDF
from .offline_offline.bosa import BOSA


def call_algo(algo_name, config, mode, device, **kwargs):
    algo_name = algo_name.lower()
    algo_to_call = {"mobody": MOBODY, "td3_bc": TD3BC, "iql": IQL, "dara": DARA, "igdf": IGDF, "bosa": BOSA}
    algo = algo_to_call[algo_name]          # KeyError for unknown names, as in the reference
    return algo(config, device)
