/*
 * deflate_l7.hip - the LZ77 stage of level 7: deflate_kernel.hip compiled with
 * that level's row of deflate_levels.h as constants
 * (lda_deflate_batch_kernel_l7; see policy_level there).
 */
#define LDA_LEVEL_INSTANCE 7
#include "deflate_kernel.hip"
