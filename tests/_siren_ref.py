"""What the SIREN fixture's generator (tests/golden/make_golden_siren.py) and its tests share: the
recipes of the inputs that are not stored (tests/golden/siren.npz holds their digests), the sampled
indices of the large tensors, and the LinearSine cases."""
import torch

ROWS = 257                      # one full 256-row tile + one ragged row
SAMPLES = 64                    # sampled entries per large gradient
ROW_STEP = 8                    # stored rows of a [257, n] output: every 8th and the last

# (key, in_features, out_features, first_layer); scales in linear_sine_scale()
LS_CASES = (("ls0", 3, 256, True), ("ls1", 259, 256, False))


def linear_sine_scale(key):
    """Constructor argument `scale` of a LinearSine case (nerf-siren/nerf_model.py:15-33)."""
    return 32.0 if key == "ls0" else torch.cat((torch.ones(256), torch.ones(3) * 32))


def linear_sine_input(key, in_features):
    """x [257, in] uniform in [-1, 1), from the case's own generator."""
    g = torch.Generator().manual_seed({"ls0": 20, "ls1": 21}[key])
    return torch.rand(ROWS, in_features, generator=g) * 2 - 1


def upstream(n_cols):
    """The fixed non-uniform upstream gradient [257, n]: linspace(0.5, 1.5) rows x cos columns."""
    w = torch.linspace(0.5, 1.5, ROWS)
    c = torch.cos(0.37 * torch.arange(n_cols, dtype=torch.float32))
    return w[:, None] * c[None, :]


def stored_rows():
    return sorted(set(range(0, ROWS, ROW_STEP)) | {ROWS - 1})


def sample_idx(numel):
    return torch.linspace(0, numel - 1, min(SAMPLES, numel)).long()


def digest(t):
    t = t.detach().double()
    return [t.sum().item(), t.abs().sum().item()]
