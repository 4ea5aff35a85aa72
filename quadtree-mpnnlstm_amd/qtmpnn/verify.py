"""The result of NextFramePredictorS2S.verify(): the products of one pass over a loader, by name and in the order asked for.

A container and nothing else: every number stays where it is defined, in the product's own result object (qtmpnn.score.Scores,
qtmpnn.reliability.Reliability, qtmpnn.fss.FSS, qtmpnn.edges.EdgeDistance, qtmpnn.extent.Extent, qtmpnn.events.EventDates, or the
array of predict)."""


class Verification:
    """`v['fss']` and `v.fss` are the result objects, each what the method of that name returns; `v.products` the names in the
    order they were asked for and computed; `v.sources` the forecast sources of the call: 'model', then the names of its
    `references` in the order asked for -- by default 'persistence' and, with a climatology, 'climatology' (event_dates lists
    'observed' first and has no persistence by default, and a product given references of its own has those: see its `.sources`).
    `name in v`, `len(v)` and iteration run over the names."""

    def __init__(self, results, sources):
        self._results = dict(results)
        self.products, self.sources = tuple(self._results), tuple(sources)

    def __getitem__(self, name):
        try:
            return self._results[name]
        except (KeyError, TypeError):
            raise KeyError(f'no product {name!r}: this verification computed {self.products}') from None

    def __getattr__(self, name):            # only reached for names that are no attribute: the products
        if name.startswith('_'):
            raise AttributeError(name)
        try:
            return self[name]
        except KeyError as e:
            raise AttributeError(e.args[0]) from None

    def __contains__(self, name):
        return name in self.products

    def __iter__(self):
        return iter(self.products)

    def __len__(self):
        return len(self.products)

    def items(self):
        return self._results.items()

    def __repr__(self):
        return f'Verification(products={self.products}, sources={self.sources})'
