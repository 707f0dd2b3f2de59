"""Cases of the LSTM-baseline and B3-MFN fixtures, shared by make_golden_lstm.py and the tests that replay them (weights and inputs
by recipe.py)."""

# sequence models alone: (fixture, class, input width D, lengths (sorted, as pack_padded_sequence wants them), T)
LSTM_SEQ_CASES = [
    ("lstm_shared_e128", "MultiLSTM", 96, [12, 9, 6], 12),          # E = 128, H = 256, L = 5; padding changes the time softmax
    ("lstm_b1_default", "MultiLSTMB1", 1024, [7, 5], 7),           # B1's copy at its defaults: E = 512, H = 256, L = 5
]
# raw windows -> valence: (fixture, class, mods, raw dims, lengths, T, words per window)
LSTM_WINDOW_CASES = [
    ("lstm_cnn_b1", "MultiCNNLSTM", ["linguistic"], {"linguistic": 1024}, [4, 3], 4, {"linguistic": 5}),          # B1 config: F = 1024
    ("lstm_cnn_checkpoint", "MultiCNNLSTM:checkpoint", ["linguistic"], {"linguistic": 300}, [6, 4], 6, {"linguistic": 6}),
    ("b3_cnn_avl", "MultiCNNTransformerB3", ["acoustic", "image", "linguistic"],
     {"linguistic": 300, "emotient": 20, "acoustic": 88, "image": 1000}, [6, 4], 6, {"linguistic": 33, "acoustic": 10, "image": 30}),
]
# B3 sequence model alone on window embeddings (recipe.EMBED_AVL widths): (fixture, lengths, T)
B3_SEQ_CASE = ("b3_mt_avl", [10, 7, 3], 10)
