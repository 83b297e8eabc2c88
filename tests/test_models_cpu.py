"""Product nn.Module surface on the CPU (rollout path): state_dict compatibility with the reference,
CPU forward vs the golden vectors, the C-ABI library loads and exports every declared symbol.  CPU only."""
import os
import re

import numpy as np
import pytest
import torch

import helpers
from drl_urban_planning_amd import native


@pytest.mark.parametrize('name', ['case_a', 'case_b', 'case_m', 'case_k'])
def test_state_dict_keys_and_shapes_match_reference(name):
    z, sd, _ = helpers.load_case(name)
    cfg = helpers.make_cfg(**helpers.CASE_MODEL[name])
    _, _, ac = helpers.build_product(cfg, mlp=name in helpers.MLP_CASES)
    mine = ac.state_dict()
    assert list(mine.keys()) == list(sd.keys())
    for k in sd:
        assert tuple(mine[k].shape) == tuple(sd[k].shape), k
    ac.load_state_dict(sd)          # a reference checkpoint loads


@pytest.mark.parametrize('name', ['case_a', 'case_b', 'case_c', 'case_m', 'case_k'])
def test_cpu_rollout_path_matches_reference(name):
    z, sd, states = helpers.load_case(name)
    cfg = helpers.make_cfg(**helpers.CASE_MODEL[name])
    policy_net, value_net, ac = helpers.build_product(cfg, mlp=name in helpers.MLP_CASES)
    ac.load_state_dict(sd)
    B = z['fwd/value'].shape[0]
    xs = [[torch.tensor(f) for f in s] for s in states[:B]]
    actions = torch.from_numpy(z['actions'][:B]).float()
    with torch.no_grad():
        value = value_net(xs)
        logp, ent = policy_net.get_log_prob_entropy(xs, actions)
        greedy = policy_net.select_action(xs, mean_action=True)
    np.testing.assert_allclose(value.numpy(), z['fwd/value'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(logp.numpy(), z['fwd/logp'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ent.numpy(), z['fwd/entropy'], rtol=1e-5, atol=1e-5)
    # greedy actions point at valid candidates of the right stage
    for b in range(B):
        st = int(np.argmax(states[b][8]))
        if st == 0:
            assert states[b][6][int(greedy[b, 0])]
        elif st == 1:
            assert states[b][7][int(greedy[b, 1])]


def test_update_refuses_cpu():
    from drl_urban_planning_amd import PPOUpdater, synth
    cfg = helpers.make_cfg(**helpers.CASE_MODEL['case_a'])
    policy_net, value_net, _ = helpers.build_product(cfg)
    up = PPOUpdater(policy_net, value_net, mini_batch_size=4)
    _, _, states = helpers.load_case('case_a')
    z = np.load(os.path.join(helpers.GOLDEN, 'case_a.npz'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        up.update_params(synth.Replay(states, z['actions'], z['masks'], z['rewards'], z['exps']))


def test_library_exports_every_declared_symbol(repo_root):
    header = open(os.path.join(repo_root, 'include', 'upamd.h')).read()
    declared = set(re.findall(r'\b(upamd_[a-z0-9_]+)\s*\(', header))
    assert declared == set(native.SYMBOLS.keys())
    lib = native.lib()              # loads, binds and version-checks every symbol
    assert lib.upamd_abi_version() == native.ABI_VERSION


def test_param_table_covers_state_dict():
    cfg = helpers.make_cfg(**helpers.CASE_MODEL['case_b'])
    policy_net, value_net, ac = helpers.build_product(cfg)
    desc = native.make_desc(cfg.state_encoder_specs, cfg.policy_specs, cfg.value_specs, 23, 52)
    table, n_floats, groups = native.param_table(desc)
    from drl_urban_planning_amd.models import backend_of
    named = backend_of(policy_net).named_params()
    assert set(named) == {t[0] for t in table}
    for name, off, rows, cols, grp in table:
        assert named[name].numel() == rows * cols, name
        assert off % 4 == 0
    assert sum(p.numel() for p in ac.parameters()) <= n_floats
    assert groups[0][0] == 0 and groups[2][1] == n_floats


def test_param_table_of_the_mlp_encoder():
    """rl-mlp (MLPStateEncoder): numerical + node encoder + heads only; the value head sees 2D + S + 3 columns."""
    name = 'case_m'
    cfg = helpers.make_cfg(**helpers.CASE_MODEL[name])
    policy_net, value_net, ac = helpers.build_product(cfg, mlp=True)
    from drl_urban_planning_amd.models import backend_of
    backend = backend_of(policy_net)
    table, n_floats, groups = native.param_table(backend.desc())
    named = backend.named_params()
    assert set(named) == {t[0] for t in table}
    assert not any('attention' in t[0] or 'edge_fc' in t[0] for t in table)
    D = helpers.CASE_MODEL[name]['D']
    assert dict((t[0], (t[2], t[3])) for t in table)['value_head.linear_0.weight'] == (32, 2 * D + 16 + 3)


def test_unsupported_configs_fail_loudly():
    cfg = helpers.make_cfg(D=24)
    with pytest.raises(RuntimeError, match='multiple of 16'):
        native.param_table(native.make_desc(cfg.state_encoder_specs, cfg.policy_specs, cfg.value_specs, 23, 52))
    cfg = helpers.make_cfg()
    cfg.state_encoder_specs['num_edge_fc_layers'] = 5
    with pytest.raises(NotImplementedError):
        native.make_desc(cfg.state_encoder_specs, cfg.policy_specs, cfg.value_specs, 23, 52)


def test_param_table_lists_the_edge_mlp_sublayers():
    # num_edge_fc_layers > 1 (state_encoder.py:59-82): linear_1 .. linear_K-1 are [D, D] tensors of the shared group,
    # named like the reference's state_dict keys; K = 1 keeps the old table
    cfg = helpers.make_cfg(D=32, L=2, K=3)
    table, n_floats, groups = native.param_table(native.make_desc(cfg.state_encoder_specs, cfg.policy_specs, cfg.value_specs, 23, 52))
    shapes = dict((t[0], (t[2], t[3], t[4])) for t in table)
    for l in range(2):
        assert shapes['shared_net.edge_fc_layers.%d.linear_0.weight' % l] == (32, 64, 0)
        for k in (1, 2):
            assert shapes['shared_net.edge_fc_layers.%d.linear_%d.weight' % (l, k)] == (32, 32, 0)
            assert shapes['shared_net.edge_fc_layers.%d.linear_%d.bias' % (l, k)] == (32, 1, 0)
    _, _, ac = helpers.build_product(cfg)
    names = set(k.split('.', 1)[1] for k in ac.state_dict() if 'shared_net' in k)
    assert set(n for n in shapes if n.startswith('shared_net.')) == names
    cfg1 = helpers.make_cfg(D=32, L=2)
    table1, n1, _ = native.param_table(native.make_desc(cfg1.state_encoder_specs, cfg1.policy_specs, cfg1.value_specs, 23, 52))
    assert n_floats - n1 == 2 * 2 * (32 * 32 + 32) and not any('linear_1' in t[0] and 'edge_fc' in t[0] for t in table1)


def test_workspace_plan_of_a_deep_edge_mlp_model():
    # host-side only (no launch): a K > 1 model plans the per-incidence tensors from the minibatch's n_inc, names the
    # sub-layer activations for the stage tests, and K = 1 models ignore n_inc
    import ctypes as C
    L = native.lib()

    def plan(K, n_inc, name=None):
        cfg = helpers.make_cfg(D=32, L=2, K=K)
        d = native.make_desc(cfg.state_encoder_specs, cfg.policy_specs, cfg.value_specs, 23, 52)
        h = C.c_void_p()
        native.check(L.upamd_engine_create(C.byref(d), C.byref(h)), 'upamd_engine_create')
        mb = native.Minibatch()
        mb.B, mb.n_nodes, mb.n_he, mb.n_rn, mb.max_n, mb.max_inc, mb.n_inc = 4, 100, 50, 20, 30, 120, n_inc
        b = C.c_int64()
        native.check(L.upamd_workspace_bytes(h, C.byref(mb), 1, C.byref(b)), 'upamd_workspace_bytes')
        out = [b.value]
        if name:
            off, r, c, k = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
            out.append(L.upamd_ws_tensor(h, C.byref(mb), name.encode(), C.byref(off), C.byref(r), C.byref(c), C.byref(k)))
            out += [r.value, c.value, k.value]
        L.upamd_engine_destroy(h)
        return out
    assert plan(1, 400) == plan(1, 0)
    two = plan(2, 400, 'EA2_2')
    assert two[0] > plan(1, 400)[0] and two[1:] == [0, 400, 32, 1]
    assert plan(2, 4000)[0] - two[0] >= 3600 * 32 * 4 * (2 * 2 + 2)      # A_k of both layers + the backward ping-pong
    assert plan(2, 400, 'EA2_3')[1] != 0 and plan(3, 400, 'EA2_3')[1] == 0


def test_kernel_lab_knobs_per_engine_bracket():
    """The library's kernel-lab knobs are process-wide (upamd_tune); ``native.tuned(overrides)`` -- the bracket NativeEngine puts
    around ITS native calls (``engine.set_tune``) -- makes them per engine: inside the block the overrides hold, behind it the process
    defaults are back, and two threads with different overrides each see their own (only the enqueue is serialised).  Checked on
    the one decision that needs no GPU: whether a minibatch takes the fused small-model path (tiny_fused)."""
    import ctypes as C
    import threading
    L = native.lib()
    cfg = helpers.make_cfg(D=16, L=2)
    d = native.make_desc(cfg.state_encoder_specs, cfg.policy_specs, cfg.value_specs, 23, 52)
    h = C.c_void_p()
    native.check(L.upamd_engine_create(C.byref(d), C.byref(h)), 'upamd_engine_create')
    mb = native.Minibatch()
    mb.B, mb.n_nodes, mb.n_he, mb.n_rn, mb.max_n, mb.max_inc, mb.max_cand = 4, 100, 50, 0, 30, 120, 20
    fused = lambda: L.upamd_step_fused_ok(h, C.byref(mb))
    assert fused() == 1
    with native.tuned({'tiny_fused': 0}):
        assert fused() == 0
        with native.tuned({}):                      # an engine without overrides inside: nothing changes, nothing is restored
            assert fused() == 0
        with native.tuned({'tiny_fused': 0}):       # the same engine's nested call: the INNER bracket must not restore anything
            assert fused() == 0
        assert fused() == 0
    assert fused() == 1
    native.tune('tiny_fused', 0)                    # a PROCESS default: what engines without their own setting see ...
    try:
        assert fused() == 0
        with native.tuned({'tiny_fused': 1}):       # ... and what the bracket of an engine WITH one restores behind itself
            assert fused() == 1
        assert fused() == 0
    finally:
        native.tune('tiny_fused', 1)
    assert fused() == 1
    # unknown knobs and retired lab settings are refused, not clamped to a default: the wrapper knows no such knob (KeyError), or
    # the library answers UPAMD_E_INVALID (RuntimeError) -- and refuses them itself as well
    for name, value in (('no_such_knob', 1), ('side_priority', 1), ('gemm_nt_dma', 2), ('gemm_nt_dma', 9), ('side_wgrad', 2),
                        ('side_wgrad', 3), ('fold_layer1', 2)):
        with pytest.raises((KeyError, RuntimeError)):
            native.tune(name, value)
        assert native.lib().upamd_tune(name.encode(), value) == -1, (name, value)      # UPAMD_E_INVALID
    seen = {0: set(), 1: set()}

    def worker(v):
        for _ in range(300):
            with native.tuned({'tiny_fused': v}):
                seen[v].add(fused())
    ts = [threading.Thread(target=worker, args=(v,)) for v in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert seen == {0: {0}, 1: {1}} and fused() == 1
    L.upamd_engine_destroy(h)
