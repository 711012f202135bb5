/*
 * tar_write_kernels.hip - a tar archive written into device memory from the
 * rows of tar_write_plan.h (host_tar_write.hip launches it; what the bytes
 * are: include/libdeflate_amd.h).
 *
 *   lda_tarw_pack_kernel   ONE kernel writes the whole archive.  Every block
 *                          of 512 bytes is a pure function of the plan: a pax
 *                          header, a block of pax data, an entry's header, a
 *                          block of its data, or zeros.  A workgroup takes one
 *                          tile of 64 KiB of the ARCHIVE - not of the entries,
 *                          as the reader's gather does -: it searches the
 *                          entries' offsets once, for the entry that holds
 *                          its tile's first block, and then walks forward
 *                          entry by entry to the tile's end with one row read
 *                          each, so many small entries share one search.  The
 *                          walk is uniform in the workgroup.  Tiles begin at
 *                          multiples of 512, so a header block never straddles
 *                          two; a run of pax data or of an entry's data may,
 *                          and each side writes the blocks that are its own.
 *                          So every byte of [0, total) is written exactly once
 *                          and none outside.  (One workgroup per tile and not
 *                          a grid that strides: the loop over tiles cost more
 *                          scalar registers than there are.)
 *
 *                          A header block is built by a wave: 64 lanes of 8
 *                          bytes, the octal digits per lane, the checksum a
 *                          wave sum with the field counted as spaces
 *                          (lda_tar_scan_kernel checks it the same way), one
 *                          8-byte store per lane.  The tile's h-th header goes
 *                          to wave h & 3.  Data is the reader's copy_tile()
 *                          (tar_copy.h) by all four waves, sources and d_out
 *                          at any alignment; padding, record padding and the
 *                          archive's end are zero_tile().
 *
 * The plan is the host's own arithmetic, not input from a file: the kernel
 * trusts it, and every store lies in [t0, t1) of the workgroup's tile.
 */
#include "device_common.h"
#include "kernels.h"
#include "tar_copy.h"

#define BLOCK 512u
#define TILE ((u64)LDA_TARW_TILE)
#define NAME_FIELD 100u

/* "0000644\0" and "0000000\0"; "ustar\0" "00"; "././@Pax" "Header\0\0" */
#define MODE_FILE 0x0034343630303030ull
#define MODE_ZERO 0x0030303030303030ull
#define MAGIC 0x3030007261747375ull
#define PAX_NAME0 0x786150402F2E2F2Eull
#define PAX_NAME1 0x0000726564616548ull

static __device__ __forceinline__ u32 byte_of(u64 v, u32 i)
{
	return (u32)(v >> (8 * i)) & 0xFF;
}

static __device__ __forceinline__ u64 blocks_of(u64 bytes)
{
	return (bytes + BLOCK - 1) / BLOCK;
}

/* decimal digits of a pax record's length (at most 65 535 + 13) */
static __device__ __forceinline__ u32 dec_digits(u32 v)
{
	return 1 + (v >= 10) + (v >= 100) + (v >= 1000) + (v >= 10000);
}

/* the lane's 8 bytes of a header's name field from a name that fits it as it
 * stands: name[8 lane .. 8 lane + 8), 0 past its end */
static __device__ __forceinline__ u64
name_plain(const u8 *__restrict__ name, u32 len, u32 lane)
{
	u64 v = 0;
#pragma unroll
	for (u32 i = 0; i < 8; i++) {
		const u32 at = 8 * lane + i;
		if (at < len)
			v |= (u64)name[at] << (8 * i);
	}
	return v;
}

/*
 * The same of a name with a pax record: its first 100 CHARACTERS, every
 * character that is not ASCII as one '?' - a lead byte becomes '?', a
 * continuation byte is dropped.  100 characters lie in the first 400 bytes:
 * every lane takes 8 of the first 512, a wave scan numbers the characters, and
 * they meet in the wave's 104 bytes of LDS.
 */
static __device__ __forceinline__ u64
name_short(const u8 *__restrict__ name, u32 len, u32 lane, u64 *stage)
{
	u8 *chars = (u8 *)stage;
	u8 b[8];
	u32 mine = 0;

	if (lane < 13)
		stage[lane] = 0;
#pragma unroll
	for (u32 i = 0; i < 8; i++) {
		const u32 at = 8 * lane + i;
		b[i] = at < len ? name[at] : 0x80;	/* (past the end: nothing) */
		mine += (b[i] & 0xC0) != 0x80;
	}
	u32 c = wave_scan_incl(mine) - mine;
	wave_sync();
#pragma unroll
	for (u32 i = 0; i < 8; i++)
		if ((b[i] & 0xC0) != 0x80) {
			if (c < NAME_FIELD)
				chars[c] = b[i] < 0x80 ? b[i] : '?';
			c++;
		}
	wave_sync();
	const u64 v = lane < 13 ? stage[lane] : 0;
	wave_sync();	/* (the wave's next header clears the bytes) */
	return v;
}

/* `count` of the 11 octal digits of f, from digit `first` (0: the most
 * significant), as ASCII in ascending bytes */
static __device__ __forceinline__ u64 oct_bytes(u64 f, u32 first, u32 count)
{
	u64 r = 0;
#pragma unroll
	for (u32 i = 0; i < count; i++)
		r |= (u64)(0x30 + ((u32)(f >> (3 * (10 - first - i))) & 7)) << (8 * i);
	return r;
}

/*
 * One header block at blk by a wave: the name field from name8 (the lane's 8
 * bytes of it, 0 in the lanes past the field and in the bytes past 100), mode,
 * uid, gid, size and mtime in octal, the checksum, the typeflag, the magic.
 * The fields from byte 100 to the typeflag are eight words of 8 bytes that
 * begin in the middle of lane 12's: lane 12 + j forms word j, and a lane's
 * bytes are the upper half of the word below and the lower half of its own.
 */
static __device__ __forceinline__ void
header_block(u8 *__restrict__ blk, u64 name8, u64 mode, u64 size, u64 mtime, u32 typeflag,
	     u32 lane)
{
	const u32 j = lane - 12;
	u64 w = 0;

	w = j == 0 ? mode : w;
	w = j == 1 || j == 2 ? MODE_ZERO : w;	/* uid, gid */
	w = j == 3 ? oct_bytes(size, 0, 8) : w;	/* 11 digits and a NUL, twice */
	w = j == 4 ? oct_bytes(size, 8, 3) | oct_bytes(mtime, 0, 4) << 32 : w;
	w = j == 5 ? oct_bytes(mtime, 4, 7) : w;
	w = j == 6 ? 0x2020202020202020ull : w;	/* the checksum counts as spaces */
	w = j == 7 ? typeflag : w;
	const u64 below = (u64)__shfl_up((u32)(w >> 32), 1, 64);
	u64 v = name8 | below | w << 32;
	v |= lane == 32 ? MAGIC << 8 : lane == 33 ? MAGIC >> 56 : 0;	/* bytes 257 .. 264 */
	u32 sum = 0;
#pragma unroll
	for (u32 i = 0; i < 8; i++)
		sum += byte_of(v, i);
	sum = wave_sum(sum);	/* at most 512 x 255: six octal digits */
	/* "%06o\0 " at 148: lanes 18 and 19 hold four bytes of it each */
	if (lane == 18 || lane == 19) {
		u64 f = 0;
#pragma unroll
		for (u32 d = 0; d < 6; d++)
			f |= (u64)(0x30 + ((sum >> (3 * (5 - d))) & 7)) << (8 * d);
		f |= (u64)0x20 << 56;
		v = lane == 18 ? (v & 0xFFFFFFFFull) | f << 32 : (v & ~0xFFFFFFFFull) | f >> 32;
	}
	__builtin_memcpy(blk + 8 * lane, &v, 8);	/* d_out has any alignment */
}

/*
 * Workgroup t writes bytes [65536 t, 65536 (t + 1)) of the archive of n entries
 * in out[0 .. total): `end` is where the last entry ends, total the size
 * (tar_write_plan.h: both from the host).  rows: the plan's rows, LDA_TARW_ECOLS
 * words per entry (LDA_TARW_E_*): entry k begins at OFF (ascending, 0 for entry
 * 0); PAX is the length of its pax record or 0; its name is names[NAME_OFF ..
 * + NAME_LEN) and its bytes are in[SRC .. + SIZE).
 */
extern "C" __global__ void __launch_bounds__(256)
lda_tarw_pack_kernel(u64 n, u64 end, u64 total, u64 mtime, const u64 *__restrict__ rows,
		     const u8 *__restrict__ names, const u8 *__restrict__ in,
		     u8 *__restrict__ out)
{
	__shared__ u64 stage[4][13];
	u32 tid = threadIdx.x;
	const u64 t0 = blockIdx.x * TILE, t1 = t0 + TILE < total ? t0 + TILE : total;
	u32 h = 0;	/* headers of the tile so far */

	/* the two end blocks and the record's rest */
	const u64 z = end > t0 ? end : t0;
	if (z < t1)
		zero_tile(out + z, (u32)(t1 - z), tid);
	if (t0 >= end)	/* (else n != 0) */
		return;
	/* the last entry that begins at or below t0 holds t0; from there on all
	 * of the walk is uniform in the workgroup */
	u64 lo = 0, hi = n;
	for (u32 s = 0; s < 64 && hi - lo > 1; s++) {
		const u64 mid = lo + (hi - lo) / 2;
		if (rows[LDA_TARW_ECOLS * mid + LDA_TARW_E_OFF] <= t0)
			lo = mid;
		else
			hi = mid;
	}
	u64 at = rows[LDA_TARW_ECOLS * lo + LDA_TARW_E_OFF];
	for (u64 k = lo; k < n && at < t1; k++) {
		const u64 *row = rows + LDA_TARW_ECOLS * k;
		const u64 e_name = row[LDA_TARW_E_NAME_OFF], e_src = row[LDA_TARW_E_SRC];
		const u64 e_size = row[LDA_TARW_E_SIZE];
		const u32 e_pax = (u32)row[LDA_TARW_E_PAX];
		const u32 e_len = (u32)row[LDA_TARW_E_NAME_LEN];
		const u8 *name = names + e_name;
		const u32 dg = dec_digits(e_pax);

		/* an entry is one record or two, each a header block and data: the
		 * pax record "%d path=%s\n" (ext) around the name's bytes, then the
		 * entry's own bytes */
		for (u32 part = e_pax ? 0 : 1; part < 2; part++) {
			const bool ext = part == 0;
			const u32 pre = ext ? dg + 6 : 0;
			const u64 len = ext ? e_len : e_size, size = ext ? e_pax : e_size;
			const u8 *from = ext ? name : in + e_src;
			const u64 hdr = at, data = hdr + BLOCK;
			const u64 next = data + blocks_of(size) * BLOCK;
			/* (the thread's number is made opaque per record: what
			 * depends on it alone - a dozen lane masks of the header's
			 * fields, the copies' offsets - would otherwise be formed
			 * once in front of the loops and held in scalar registers
			 * through the whole kernel, more than it has) */
			asm volatile("" : "+v"(tid));
			const u32 lane = tid & 63, wave = tid >> 6;

			if (hdr >= t0 && hdr < t1 && (h++ & 3) == wave) {
				const u64 name8 =
					ext ? (lane == 0 ? PAX_NAME0 : lane == 1 ? PAX_NAME1 : 0) :
					e_pax ? name_short(name, e_len, lane, stage[wave]) :
						name_plain(name, e_len, lane);
				header_block(out + hdr, name8, ext ? MODE_ZERO : MODE_FILE, size,
					     ext ? 0 : mtime, ext ? 'x' : '0', lane);
			}
			if (data >= t0 && data < t1 && tid < pre) {	/* "%d path=" */
				u32 v = e_pax;
				for (u32 j = dg - 1; j > tid; j--)
					v /= 10;
				out[data + tid] = tid < dg ? 0x30 + v % 10 :
						  byte_of(0x3D6874617020ull, tid - dg);
			}
			/* (a pad is shorter than a block: it lies in one tile) */
			const u64 ps = data + size;
			if (ext && ps - 1 >= t0 && ps - 1 < t1 && tid == 0)
				out[ps - 1] = 0x0A;
			if (ps < next && ps >= t0 && ps < t1)
				zero_tile(out + ps, (u32)(next - ps), tid);
			at = next;
			const u64 body = data + pre;
			const u64 a = body > t0 ? body : t0;
			const u64 b = body + len < t1 ? body + len : t1;
			if (a < b)
				copy_tile(from + (a - body), out + a, b - a, tid);
		}
	}
}
