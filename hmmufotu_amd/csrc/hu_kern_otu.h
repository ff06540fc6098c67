// hmmufotu-subset's multinomial method on the device (src/OTUTable.cpp:189-209): with replacement, a lane per draw; the
// read it names (hu_otu_draw) is looked up by binary search of the sample's prefixes.  The lists are those of the uniform method
// (hu_draw.h), a chunk being chunkLen draws; integer atomics only.
#pragma once
#include "hu_kern_draw.h"

/* grid: the chunks of the groups; a lane per draw of the multinomial method, chunkLen draws to a workgroup, `size` to a sample */
static __global__ __launch_bounds__(HU_DRAW_WG) void k_otu_multinom(const HuAlSample* smp, const HuAlDraw* draw, const HuAlGroup* grp, const HuAlChunk* chunk,
		const uint32_t* prefix, uint32_t* out, int chunkLen, uint32_t size) {
	const HuAlChunk c = chunk[blockIdx.x];
	const HuAlGroup g = grp[c.g];
	const HuAlSample s = smp[g.smp];
	const int lane = threadIdx.x & 63;
	const uint32_t* P = prefix + s.pfx0;
	uint32_t* o = out + draw[g.draw0].cell0;
	const uint32_t key[2] = {g.k0, g.k1};
	const uint64_t end = min((uint64_t) c.t0 + (uint64_t) chunkLen, (uint64_t) size);
	for(uint64_t base = c.t0; base < end; base += HU_DRAW_WG) {
		const uint64_t m = base + threadIdx.x;
		const bool valid = m < end;
		uint32_t cell = 0xffffffffu;
		if(valid) cell = hu_draw_cell(P, s.nnz, (uint32_t) hu_otu_draw(key, m, s.col, s.T));
		/* a wave whose draws all fall into one cell (a sample that one OTU holds) adds once */
		const uint64_t vm = __ballot(valid);
		if(!vm) continue;
		const int firstLane = __ffsll((unsigned long long) vm) - 1;
		const uint32_t c0 = __shfl(cell, firstLane);
		if(__ballot(valid && cell == c0) == vm) { if(lane == firstLane) atomicAdd(&o[c0], (uint32_t) __popcll(vm)); }
		else if(valid) atomicAdd(&o[cell], 1u);
	}
}
