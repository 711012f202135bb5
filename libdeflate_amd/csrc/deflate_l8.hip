/*
 * deflate_l8.hip - the LZ77 stage of level 8: deflate_kernel.hip compiled with
 * that level's row of deflate_levels.h as constants
 * (lda_deflate_batch_kernel_l8; see policy_level there).
 */
#define LDA_LEVEL_INSTANCE 8
#include "deflate_kernel.hip"
