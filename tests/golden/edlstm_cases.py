"""Cases of the encoder-decoder LSTM fixtures (MultiEDLSTM, transformer/MFT/models.py:222-308), shared by make_golden_edlstm.py and the
tests that replay them (weights and inputs by recipe.py)."""

# (fixture, input width D, constructor keywords, lengths (sorted, as pack_padded_sequence wants them), T, tgt_init)
EDLSTM_CASES = [
    ("lstm_ed_default", 96, dict(embed_dim=128, h_dim=128, attn_len=3), [12, 9, 6], 12, 0.0),       # the largest sizes the scan takes
    ("lstm_ed_h40", 48, dict(embed_dim=24, h_dim=40, attn_len=2), [7, 5], 7, 0.5),                  # padded units and read-out rows
    ("lstm_ed_e128_h64", 64, dict(embed_dim=128, h_dim=64), [5, 5], 5, -0.25),                      # E > H; the class's attn_len
]
