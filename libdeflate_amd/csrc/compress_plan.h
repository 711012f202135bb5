/*
 * compress_plan.h - the arithmetic of one compress batch call
 * (host_compress.hip, compress_batch_impl()): which kernel a batch takes, how
 * it is cut into scratch-limited slices, where the kernels' scratch regions
 * lie, and how a slice of the split path is cut into a head and a tail that
 * run on two streams.  A pure function of its arguments, so that a host
 * compiler takes it alone (tools/test_compress_plan.cpp).
 */
#ifndef LDA_COMPRESS_PLAN_H
#define LDA_COMPRESS_PLAN_H

#include <stddef.h>
#include <stdint.h>

namespace lda {

/*
 * The split path's scratch (kernels.h, LDA_BLK_*) is at most this much per
 * launch: 4 B of token list per byte of the size bound plus the block
 * descriptors, so 4096 buffers of 64 KiB (1.08 GiB) are one launch.  A batch
 * that needs more runs as consecutive slices of buffers on the same stream; a
 * bound whose single buffer needs more keeps the fused kernel.  (The tail's
 * second descriptor region and workgroup state, below, come on top: 5.6 MiB
 * for 256 buffers of 64 KiB.)
 */
#define LDA_SPLIT_SCRATCH ((size_t)1280 << 20)
/* buffers per CU from which a call takes the split path (see plan_batch());
 * a tuning build may set another (make VARIANT=... EXTRA=-DLDA_SPLIT_MIN_PER_CU=1) */
#ifndef LDA_SPLIT_MIN_PER_CU
#define LDA_SPLIT_MIN_PER_CU 4
#endif
/*
 * Buffers per CU of a slice's tail (R, LDA_COMPRESS_TAIL_ROUNDS).  Measured
 * (profiles/r15_overlap.md; three runs each, alternated in one job), ms per
 * step of the bench batch (4096 x 64 KiB gzip level 6, compress + decompress):
 *   serial 7.783 / 7.801 / 7.802
 *   R = 1  7.701 / 7.713 / 7.713
 *   R = 2  7.715 / 7.727 / 7.705
 *   R = 4  7.709 / 7.723 / 7.732
 * A longer tail only makes the tail's own entropy launch longer: the head's
 * entropy launch cannot start before the head's last workgroup has left, and
 * that is when the tail's last buffer starts, whatever R.  1024 x 64 KiB (4
 * buffers per CU on 256 CUs) has no tail at any R - the head would keep fewer
 * than LDA_SPLIT_MIN_PER_CU - and measures 1.69 ms per call at level 6 with
 * R = 1, 2, 4 and on the serial schedule alike.
 */
#ifndef LDA_COMPRESS_TAIL_ROUNDS
#define LDA_COMPRESS_TAIL_ROUNDS 1
#endif
/* the block descriptors' layout (kernels.h: LDA_BLK_WORDS, LDA_BLK_LIST,
 * LDA_BLK_HDR_WORDS; host_compress.hip asserts that they agree) */
#define LDA_PLAN_BLK_WORDS 328
#define LDA_PLAN_BLK_LIST(n) (((n) + 15) / 16 * 16)
#define LDA_PLAN_BLK_HDR_WORDS(n) (2 * LDA_PLAN_BLK_LIST(n))

/* what the plan takes from the device and the kernels */
struct compress_plan_env {
	size_t num_cus;
	/* the small-buffer kernel (deflate_small.hip): largest buffer, workgroups
	 * per CU, LDA_NO_SMALL */
	size_t small_max, small_wgs;
	bool no_small;
	size_t tile;		/* lda_deflate_tile() */
	size_t seq_words;	/* lda_deflate_seq_words(): u64 of state per workgroup */
	size_t dict_bytes;	/* the dictionary block: LDA_DICT_BLK_HDR + dict_window() */
	size_t tail_rounds;	/* R; 0: the serial schedule */
};

/*
 * The kernels' scratch of one compress_batch_impl() call: [per-workgroup
 * state: u64 x seq_words x grid, then the same x grid2 for the tail's LZ77
 * launch][chunk counters: four u32 per slice (the LZ77 stage's, the fused
 * kernel's behind it, the count of buffers left to that one, the entropy
 * kernel's), then the tail's four per slice][sums: u32 x n], then the
 * dictionary block (see lda_dict_prep_kernel()) or, on the split path, one
 * slice's token lists and block descriptors and, behind them, the tail's block
 * descriptors.  The same sum sizes the reservations the host-pointer entry
 * points make up front.  A call that does not overlap has grid2 = 0 and no
 * tail regions: the layout of the serial schedule.
 */
struct batch_plan {
	bool small, split;
	size_t grid, per_slice, nslices;
	uint32_t tok_stride, blk_stride;	/* u32 entries / descriptors per buffer */
	size_t cnt_at, sums_at, tok_at, blk_at, dict_at, total;
	/* the tail (overlap: some slice of the call has one) */
	bool overlap;
	size_t tail_rounds, tail_max, grid2;
	size_t seq2_at, cnt2_at, blk2_at;
};

static inline size_t plan_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/*
 * The tail of a slice of nk buffers: the last R buffers per CU, where that
 * leaves the head at least what a split launch asks for; otherwise none (the
 * slice runs on the serial schedule).
 */
static inline size_t plan_tail_of(size_t nk, size_t num_cus, size_t R)
{
	if (!R || nk / num_cus < LDA_SPLIT_MIN_PER_CU + R)
		return 0;
	return R * num_cus;
}

static inline batch_plan plan_batch(const compress_plan_env &e, size_t n, size_t max_in, int level,
				    bool seg, bool dict)
{
	batch_plan p = {};
	/* buffers of at most 4 KiB (filesystem blocks): the 256-thread kernel,
	 * several workgroups per CU (deflate_small.hip); levels 10-12 keep the
	 * big one (their parse wants its LDS); a dictionary needs the ring of
	 * the big kernel */
	p.small = max_in <= e.small_max && level <= 9 && !seg && !dict && !e.no_small;
	/* levels 0-9 of the big kernel split the block end off into the entropy
	 * kernel (deflate_entropy.hip) wherever the host knows a size bound to
	 * size the token lists by, and the call has buffers enough to fill the
	 * CUs several times over: the entropy kernel's work per buffer (0.11 ms
	 * for 64 KiB at level 6: 0.42 ms per 4096 of the bench mix, four to a
	 * CU; 0.19 before round 9) is what the split saves only where other
	 * buffers' block ends run beside it - with one buffer per CU it is a tail
	 * the fused kernel does not have (4096 x 64 KiB: 7.16 -> 6.57 ms in
	 * round 7, 6.23 in round 9).  A 16 MiB single-buffer call (256
	 * segments) forced onto the split path measured 1.24 -> 1.49 ms in round
	 * 7; in round 9 fused and split are 1.26 - 1.39 and 1.29 - 1.40 ms, inside
	 * each other's spread, so the threshold stays */
	const size_t tile = e.tile;
	const size_t tok_stride = plan_align_up(max_in, 16);
	const size_t blk_tiles = (tok_stride + tile - 1) / tile;
	const size_t blk_stride = blk_tiles ? blk_tiles : 1;
	const size_t per_buf = tok_stride * 4 + blk_stride * LDA_PLAN_BLK_WORDS * 4 + 4;
	const size_t num_cus = e.num_cus;
	p.split = !p.small && level <= 9 && !dict && max_in != SIZE_MAX &&
		  n >= LDA_SPLIT_MIN_PER_CU * num_cus &&
		  per_buf <= LDA_SPLIT_SCRATCH && tok_stride <= 0xFFFFFFF0u;
	p.per_slice = p.split ? (n < LDA_SPLIT_SCRATCH / per_buf ? n : LDA_SPLIT_SCRATCH / per_buf) : n;
	if (p.per_slice < 1)
		p.per_slice = 1;
	p.nslices = (n + p.per_slice - 1) / p.per_slice;
	const size_t grid_max = num_cus * (p.small ? e.small_wgs : 1);
	p.grid = p.per_slice < grid_max ? p.per_slice : grid_max;
	/*
	 * The head and the tail ("the LZ77 launch's tail").  The LZ77
	 * stage is a persistent grid, one workgroup per CU, that hands buffers out
	 * from a counter, so its workgroups finish spread over one buffer's time
	 * and a CU stands idle for half of that on average: the launch of the bench
	 * batch (16 buffers per CU, 0.36 ms each) ends with about 0.18 ms of it, 3 %.
	 * The entropy kernel behind it is the work that fits a CU the moment its
	 * LZ77 workgroup has left - but every workgroup of the LZ77 stage owns the
	 * LDS of its CU, and on one stream nothing of the next kernel starts while
	 * one is left.  So a slice's last R buffers per CU (the first slice has
	 * the most: where it has no tail, none has) go through the same two
	 * kernels on a stream of the compressor's own, with their own workgroup
	 * state, counters and block descriptors: the tail's LZ77 workgroups take
	 * the CUs the head's leave, the head's entropy launch the CUs the tail's
	 * leave.  Only the tail is won: LZ77 needs 5.81 x 256 CU-ms and the entropy
	 * stage 0.42 x 256 CU-ms per bench batch, they cannot share a CU, and the
	 * sum is what it is.
	 */
	p.tail_rounds = p.split ? e.tail_rounds : 0;
	p.tail_max = plan_tail_of(p.per_slice, num_cus, p.tail_rounds);
	p.overlap = p.tail_max != 0;
	p.grid2 = p.tail_max < grid_max ? p.tail_max : grid_max;
	p.seq2_at = p.grid * e.seq_words * 8;
	p.cnt_at = p.seq2_at + p.grid2 * e.seq_words * 8;
	p.cnt2_at = p.cnt_at + 16 * p.nslices;
	p.sums_at = p.cnt2_at + (p.overlap ? 16 * p.nslices : 0);
	p.dict_at = p.tok_at = plan_align_up(p.sums_at + n * 4, 64);
	p.total = p.sums_at + n * 4;
	if (dict)
		p.total = p.dict_at + e.dict_bytes;
	if (p.split) {
		p.tok_stride = (uint32_t)tok_stride;
		p.blk_stride = (uint32_t)blk_stride;
		p.blk_at = plan_align_up(p.tok_at + p.per_slice * tok_stride * 4, 64);
		p.total = p.blk_at + (LDA_PLAN_BLK_HDR_WORDS(p.per_slice) +
				      p.per_slice * blk_stride * LDA_PLAN_BLK_WORDS) * 4;
		p.blk2_at = p.total;
		if (p.overlap) {
			p.blk2_at = plan_align_up(p.total, 64);
			p.total = p.blk2_at + (LDA_PLAN_BLK_HDR_WORDS(p.tail_max) +
					       p.tail_max * blk_stride * LDA_PLAN_BLK_WORDS) * 4;
		}
	}
	return p;
}

} /* namespace lda */

#endif /* LDA_COMPRESS_PLAN_H */
