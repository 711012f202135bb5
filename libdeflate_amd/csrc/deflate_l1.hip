/*
 * deflate_l1.hip - the LZ77 stage of level 1: deflate_kernel.hip compiled with
 * that level's row of deflate_levels.h as constants
 * (lda_deflate_batch_kernel_l1; see policy_level there).
 */
#define LDA_LEVEL_INSTANCE 1
#include "deflate_kernel.hip"
