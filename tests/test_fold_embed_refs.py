"""CPU, float64: the algebra and the host logic of the folded embed (DiTEngine.fold_embed, dit.fold_embed_weights).

x0 = [registers ; W_in y + b + pos] is read by nothing but layer 0's three cross-condition Linears, so with the hoisted layer-0 text / frames
blocks fixed over a sample() their outputs are  table(y = 0) + y_pad G^T  with G_a = (I + W_tfa[:, :D]) W_in, G_t = W_at[:, :D] W_in,
G_f = W_af[:, :D] W_in and y_pad = y in the frame rows of both halves of the CFG batch, zero in the register rows.

  test_tables_plus_y_g       random weights of a small config (dim 128, dim_text 192, dim_frames 64, C = 64, R = 4, T = 9, B = 1 and 2, CFG
                             batch with different text / frames rows per half): the identity against oracle.cross_condition on the
                             straightforward x0, all rows and both halves, 1e-12 relative to the largest output
  test_ybuf_layout           y_plane_rows: register rows never addressed, both halves hold y, every frame row exactly once; the planes
                             L.split_planes writes there sum to y within 2^-16 |y|
  test_same_grid / test_grid_cache_on_the_engine   the host-side grid cache: the same grid keeps the time conditioning and the two modulation
                             tables (no v2a_time_cond, no fp32 GEMM in the recorded calls), a changed grid, a changed dt, another plan, a
                             prepare() without fold_embed and a device-side grid recompute them"""
import pytest
import torch
import torch.nn.functional as F

from oracle import e2_cfm_oracle as O
from v2a_amd import _lib as L
from v2a_amd.dit import DiTConfig, DiTEngine, fold_embed_weights, same_grid, y_plane_rows

CFG = dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, num_channels=64, max_seq_len=64)
T = 9


@pytest.mark.parametrize("B", [1, 2])
def test_tables_plus_y_g(B):
    cfg = O.DiTConfig(**CFG)
    P = {k: v.double() for k, v in O.init_params(cfg, 3).items()}
    R, N, D, C_ = cfg.num_registers, cfg.num_registers + T, cfg.dim, cfg.num_channels
    g = torch.Generator().manual_seed(B)
    y = torch.randn(B, T, C_, generator=g, dtype=torch.float64)
    text = torch.randn(2 * B, N, cfg.dim_text, generator=g, dtype=torch.float64)          # the hoisted layer-0 blocks: any fixed rows, the
    frames = torch.randn(2 * B, N, cfg.dim_frames, generator=g, dtype=torch.float64)      # null half differs from the conditional one

    def x0(lat):
        h = F.linear(lat, P["proj_in.weight"], P["proj_in.bias"]) + P["transformer.abs_pos_emb.weight"][:T]
        h = torch.cat((P["transformer.registers"][None].expand(B, -1, -1), h), 1)
        return torch.cat((h, h), 0)                                                       # both halves of the CFG batch embed the same y

    want = O.cross_condition(P, "transformer.layers.0.1.5", x0(y), text, frames, True)
    table = O.cross_condition(P, "transformer.layers.0.1.5", x0(torch.zeros_like(y)), text, frames, True)
    y_pad = torch.zeros(2 * B * N, C_, dtype=torch.float64)
    y_pad[y_plane_rows(B, T, N, R).reshape(-1)] = y.repeat(2, 1, 1).reshape(-1, C_)
    G = fold_embed_weights(P, D)
    assert [tuple(w.shape) for w in G] == [(D, C_), (cfg.dim_text, C_), (cfg.dim_frames, C_)] and all(w.dtype == torch.float64 for w in G)
    for name, w, tab, ref in zip("atf", G, table, want):
        got = tab + (y_pad @ w.t()).reshape(2 * B, N, -1)
        err = float((got - ref).abs().max() / ref.abs().max())
        print("fold-embed identity B=%d stream %s: relative error %.2e" % (B, name, err))
        assert err < 1e-12
        assert torch.equal(got[:, :R], tab[:, :R])                                        # register rows: the table alone


@pytest.mark.parametrize("B", [1, 2])
def test_ybuf_layout(B):
    R, N, C_ = 4, 4 + T, 64
    rows = y_plane_rows(B, T, N, R)
    assert rows.shape == (2, B, T)
    flat = rows.reshape(-1)
    assert len(set(flat.tolist())) == 2 * B * T and int(flat.max()) < 2 * B * N
    assert bool(((flat % N) >= R).all())                                                  # no register row
    for k in range(2):
        for b in range(B):
            assert rows[k, b].tolist() == list(range((k * B + b) * N + R, (k * B + b + 1) * N))
    y = torch.randn(B, T, C_, generator=torch.Generator().manual_seed(7))
    buf = torch.zeros(2 * B * N, 2 * C_, dtype=torch.bfloat16)
    buf[flat] = L.split_planes(y.reshape(-1, C_)).repeat(2, 1)
    v = buf.reshape(2, B, N, 2 * C_)
    assert not bool(v[:, :, :R].any())
    assert torch.equal(v[0], v[1])
    got = v[0, :, R:, :C_].double() + v[0, :, R:, C_:].double()
    assert bool(((got - y.double()).abs() <= 2.0 ** -16 * y.double().abs()).all())


def test_same_grid():
    t, dt = torch.linspace(0, 0.75, 4), torch.full((4,), 0.25)
    cached = (t.clone(), dt.clone())
    assert same_grid(cached, t.clone(), dt.clone())
    assert same_grid(cached, t.double(), dt.double())                    # compared as the fp32 values the device tables were made from
    assert not same_grid(None, t, dt)
    assert not same_grid(cached, t + 1e-3, dt) and not same_grid(cached, t, dt * 2) and not same_grid(cached, t[:3], dt[:3])
    assert not same_grid(cached, t, None) and not same_grid((t.clone(), None), t, dt) and same_grid((t.clone(), None), t, None)
    assert not same_grid(cached, t.to("meta"), dt)                        # a device-side grid is never compared


def test_grid_cache_on_the_engine():
    import test_launch_trace as LT
    cfg = DiTConfig(**LT.SHIPPED)
    B, nc, S = 1, 16, 4
    table_calls = []

    def run(roots):
        eng = DiTEngine(cfg, LT._state_dict(cfg), device="cpu", compute="bf16x3")
        ins = {t: LT._inputs(cfg, B, t, nc, S) for t in (150, 97)}
        roots += [eng, ins]

        def prep(t, fold=True, grid=None, dt=None):
            i = ins[t]
            eng.setup(B, t, nc, S)
            n0 = len(tr_calls())
            eng.prepare(i["text"], i["roll"], i["ctx"], i["ctx_mask"], i["t"] if grid is None else grid, dt=i["dt"] if dt is None else dt,
                        fold_embed=fold)
            new = tr_calls()[n0:]
            f32 = [c for c in new if c["fn"] == "v2a_gemm" and c["args"][0]["compute_dtype"] == L.F32]
            table_calls.append((sum(c["fn"] == "v2a_time_cond" for c in new), len(f32)))

        tr_calls = lambda: trace_ref[0]
        prep(150)                                   # 0 first call: computed
        prep(150)                                   # 1 same grid: kept
        prep(150, grid=ins[150]["t"] * 0.5)         # 2 changed grid
        prep(150, dt=ins[150]["dt"] * 0.5)          # 3 changed dt (the grid of call 0 again)
        prep(97)                                    # 4 another plan: its own tables
        prep(150, dt=ins[150]["dt"] * 0.5)          # 5 back on the first plan with the grid it was last prepared for: kept
        prep(150, fold=False, dt=ins[150]["dt"] * 0.5)      # 6 a caller that does not fold: today's launches
        prep(150, dt=ins[150]["dt"] * 0.5)          # 7 ... and forgets the cache
        prep(150, dt=ins[150]["dt"] * 0.5)          # 8 kept again

    # the recorder's call list, reachable from inside `run`: _traced builds the _Trace itself, so take it from the fake library it installs
    trace_ref = []
    orig = LT._Fake.__init__

    def spy(self, trace):
        trace_ref.append(trace.calls)
        orig(self, trace)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(LT._Fake, "__init__", spy)
        LT._traced(run)
    assert table_calls == [(1, 2), (0, 0), (1, 2), (1, 2), (1, 2), (0, 0), (1, 2), (1, 2), (0, 0)], table_calls
