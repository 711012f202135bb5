/*
 * deflate_l4.hip - the LZ77 stage of level 4: deflate_kernel.hip compiled with
 * that level's row of deflate_levels.h as constants
 * (lda_deflate_batch_kernel_l4; see policy_level there).
 */
#define LDA_LEVEL_INSTANCE 4
#include "deflate_kernel.hip"
