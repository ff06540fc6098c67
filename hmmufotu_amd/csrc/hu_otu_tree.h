// The OTU tree of hmmufotu-amd-sum -t and hmmufotu-amd-merge -t (PTUnrooted::convertToNewickTree(getAncestors(otuSeen), prefix),
// src/PhyloTreeUnrooted.cpp:426-447, 1127-1133; NewickTree::write, src/NewickTree.cpp:61-77): the tree cut down to the paths from the
// OTUs to the root — a node's children are written, all of them, when one of them lies on such a path.
#pragma once
#include <functional>
#include <ostream>
#include <string>
#include <vector>
#include "../../include/hmmufotu_amd.h"

inline void hu_otu_tree_write(std::ostream& treeOut, const hu_tree_info* ti, const std::vector<int32_t>& otus, const std::string& prefix) {
	int32_t N = 0, root = 0;
	hu_tree_info_get(ti, &N, nullptr, &root, nullptr);
	std::vector<char> onPath((size_t) N, 0);                          /* getAncestors(otuSeen): the OTUs and everything above them */
	for(int32_t u : otus) for(int32_t v = u; v >= 0 && !onPath[v]; ) { onPath[v] = 1; int32_t par = -1; hu_tree_info_node(ti, v, &par, nullptr, nullptr, nullptr, nullptr, nullptr); v = par; }
	std::function<void(int32_t)> write = [&](int32_t u) {
		const int32_t* ch = nullptr; const int nc = hu_tree_info_children(ti, u, &ch);
		bool flag = false;
		for(int i = 0; i < nc; ++i) flag |= onPath[ch[i]] != 0;
		if(flag) { treeOut << '('; for(int i = 0; i < nc; ++i) { if(i) treeOut << ","; write(ch[i]); } treeOut << ')'; }
		int32_t par = -1; double len = 0;
		hu_tree_info_node(ti, u, &par, &len, nullptr, nullptr, nullptr, nullptr);
		treeOut << prefix << u << ':' << (par < 0 ? 0.0 : len);         /* NewickTree::write: the length whenever it is >= 0, at ostream's default precision */
	};
	write(root);
	treeOut << ';';
}
