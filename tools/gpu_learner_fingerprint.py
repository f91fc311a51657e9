"""Fingerprint of the learner's three step forms, each selected by size and architecture alone: 8 graph-replayed minibatch steps of one
`sgd_epoch` on seeded inputs, then the sha256 of `flat_p`, `m`, `v`, `acc` and the loss sums, one JSON line per form.  Run it on two
commits (same `ODK_LIB`) to see that a change of `ppo/learner.py` left the arithmetic alone (profiles/learner_forms/NOTES.md).
    python tools/gpu_learner_fingerprint.py [seed]"""
import os, sys, json, hashlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from open_duck_playground_amd.ppo import train as T
from open_duck_playground_amd.ppo.learner import FlatLearner
from open_duck_playground_amd.ppo.networks import PPONetworks

seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
dev = torch.device("cuda")
N, B = 64, 16
FORMS = [("indexed", 20, {}),                                                      # the reference networks, 320 rows
         ("gathered_fused", 321, {}),                                              # 5136 rows: past odk_ppo_gae_head's 5120
         ("library", 20, dict(policy_hidden=(256, 128), value_hidden=(256, 256, 64)))]


def fake_rollout(Tn, g):
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    done = (torch.rand(N, Tn, device=dev, generator=g) < 0.08).float()
    trunc = (torch.rand(N, Tn, device=dev, generator=g) < 0.5).float() * done
    return dict(obs=r(N, Tn, 101), priv=r(N, Tn, 212), raw_action=0.7 * r(N, Tn, 14), log_prob=-12 + r(N, Tn), reward=0.05 * r(N, Tn).abs(),
                done=done, truncation=trunc, last_priv=r(N, 212))


sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
for name, Tn, arch in FORMS:
    torch.manual_seed(seed)                                   # network initialisation and the entropy noise
    g = torch.Generator(device=dev).manual_seed(seed)         # the rollout and the shuffles
    data = fake_rollout(Tn, g)
    net = PPONetworks(101, 212, 14, **arch).to(dev)
    net.norm_obs.update(data["obs"]); net.norm_priv.update(data["priv"])
    cfg = T.ppo_config(); cfg.update(num_minibatches=N // B, num_updates_per_batch=2, tune_gemms=False)
    lr = FlatLearner(net, cfg, B, Tn, use_graph=True)
    T.sgd_epoch(net, None, data, cfg, g, learner=lr, meter=T.LossMeter())     # 2 x 4 minibatch steps; with a meter the sums stay in lr.losses
    torch.cuda.synchronize()
    print(json.dumps(dict(form=name, indexed=bool(lr.indexed), fused=lr.fused is not None, steps=lr.nsteps,
                          **{k: sha(getattr(lr, k)) for k in ("flat_p", "m", "v", "acc")}, losses=lr.losses.tolist())), flush=True)
    lr.close()
