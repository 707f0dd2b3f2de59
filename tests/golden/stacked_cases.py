"""Cases of the stacked-LSTM fixtures (n_layers > 1), shared by make_golden_stacked.py and the tests that replay them (weights and inputs
by recipe.py, whose dec_h0 / dec_c0 are non-zero: the reference's zero initialisation would hide a wrong initial state)."""

# decoder models: (fixture, class, reference variant, input width D, constructor keywords, lengths, T)
DECODER_CASES = [
    ("model_sft_l2", "NLPTransformer", "SFT", 64, dict(embed_dim=128, h_dim=128, N=1, h=8, n_layers=2), [12, 9, 6], 12),
    ("model_sft_l3_d40", "NLPTransformer", "SFT", 24, dict(embed_dim=40, N=1, h=4, n_layers=3), [7, 5], 7),     # H = 40: padded units
    ("model_uni_l2", "UniTransformer", "MFT", 32, dict(embed_dim=64, N=1, h=4, n_layers=2), [5, 5], 5),
]
# LSTM baselines: (fixture, class, reference variant, input width D, constructor keywords, lengths, T)
BASELINE_CASES = [
    ("lstm_shared_l2", "MultiLSTM", "SFT", 96, dict(n_layers=2), [12, 9, 6], 12),
    ("lstm_b1_l3", "MultiLSTMB1", "B1-LSTM", 64, dict(embed_dim=64, h_dim=32, n_layers=3), [7, 5], 7),
]
