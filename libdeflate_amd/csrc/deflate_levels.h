/*
 * deflate_levels.h - level -> (search depth, nice length, parse mode), the
 * policy table of lib/deflate_compress.c:3927-3979, one row per level as a
 * macro so that the host's table (host_compress.hip, k_levels) and the LZ77
 * stage's per-level instances (deflate_l1.hip ... deflate_l9.hip: the row as
 * compile-time constants, see struct policy_level in deflate_kernel.hip) read
 * the same numbers.  mode: 0 greedy, 1 lazy, 2 lazy2, 3 min-cost.
 *
 * Level 1 maps onto the same hash-chain kernel with a 2-deep search (the
 * reference's level 1 probes a 2-way bucket, lib/ht_matchfinder.h:50-55).
 * Levels 10-12 (mode 3) choose the tokens by a min-cost parse over the chain
 * search's results instead of the lazy rule (deflate_kernel.hip, "min-cost
 * parse"); the reference's binary tree match finder (lib/bt_matchfinder.h) has
 * no counterpart.
 */
#ifndef LDA_DEFLATE_LEVELS_H
#define LDA_DEFLATE_LEVELS_H

#define LDA_LEVEL_0 0, 0, 0		/* stored */
#define LDA_LEVEL_1 2, 32, 0
#define LDA_LEVEL_2 6, 10, 0		/* greedy */
#define LDA_LEVEL_3 12, 14, 0
#define LDA_LEVEL_4 16, 30, 0
#define LDA_LEVEL_5 16, 30, 1		/* lazy */
#define LDA_LEVEL_6 35, 65, 1
#define LDA_LEVEL_7 100, 130, 1
#define LDA_LEVEL_8 300, 258, 2		/* lazy2 */
#define LDA_LEVEL_9 600, 258, 2
/* 10-12: min-cost parse over every position's deepest match.  The chains
 * of a 64 KiB buffer are exhausted at ~600 steps (13 hash bits, 24 K
 * window: 600, 1000 and 2000 measured the same time and, to 0.02 %, the
 * same bytes - round 5's 600 / 1000 / 2000 were one level three times),
 * so the ladder is 150 / 300 / all of the chain: 38.4 / 45.6 / 53.0 ms
 * per 4096 x 64 KiB at 1.0062 / 1.0082 / 1.0074 x the reference's size
 * at the same level (the mix of tests/datagen.py; round 6) */
#define LDA_LEVEL_10 150, 258, 3
#define LDA_LEVEL_11 300, 258, 3
#define LDA_LEVEL_12 2000, 258, 3

#endif /* LDA_DEFLATE_LEVELS_H */
