"""Cases of the autoregressive LSTM fixtures (MultiARLSTM, transformer/MFT/models.py:310-400), shared by make_golden_arlstm.py and the
tests that replay them (weights and inputs by recipe.py)."""
import recipe as R

# (fixture, input width D, constructor keywords, lengths (sorted, as pack_padded_sequence wants them), T, tgt_init, teacher-forced)
ARLSTM_CASES = [
    ("lstm_ar_k1", 48, dict(embed_dim=24, h_dim=40, attn_len=3, ar_order=1), [9, 6, 4], 9, 0.5, False),       # the class's ar_order
    ("lstm_ar_k3", 64, dict(embed_dim=32, h_dim=64, ar_order=3), [12, 9, 5], 12, -0.25, False),               # the class's attn_len
    # teacher-forced; its tgt_init must not show anywhere (pad_shift pads the target with zeros)
    ("lstm_ar_k3_tf", 64, dict(embed_dim=32, h_dim=64, ar_order=3), [12, 9, 5], 12, 0.5, True),
    ("lstm_ar_l2", 48, dict(embed_dim=24, h_dim=32, n_layers=2, attn_len=3, ar_order=2), [8, 8, 3], 8, 0.3, False),
    ("lstm_ar_short", 32, dict(embed_dim=16, h_dim=24, attn_len=2, ar_order=4), [2, 1], 2, 0.7, False),       # T < ar_order
]


def ar_target(name, lengths, T):
    """the (B,T,1) target a teacher-forced case feeds to the model (not the loss target of the fixture, which run_case draws)"""
    return R.gen_uniform(name + ":ar_target", (len(lengths), T, 1), R.SEED) * R.prefix_mask(lengths, T)
