"""The (n_base, state_len) pairs xb_ctx_create accepts: state_len 2..5 with n_base^state_len <= 1024."""
PAIRS = [(4, 3), (5, 3), (6, 3), (4, 2), (5, 2), (6, 2), (4, 4), (5, 4), (4, 5)]
NEW_PAIRS = [p for p in PAIRS if p[1] != 3]                      # the ones no test ran before
# parametrize ids: the state_len 3 cases keep the ids they had when n_base was the only parameter
PAIR_IDS = [str(nb) if sl == 3 else "%d-sl%d" % (nb, sl) for nb, sl in PAIRS]
